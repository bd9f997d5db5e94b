"""The input readers of seqToProfile and truthEval without a GPU: BatchReader and stream_batches (host/input_stream.h) in a
stand-alone program under the sanitizers, with batches of 64 and 256 bytes -- the carry of a partial line, a partial BGZF
member and the 28 EOF bytes from one batch to the next, which the product's batches of 8 to 64 MB keep out of every quick
test's reach -- against a plain model that cuts the whole file image at boundaries."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "simuscop_amd", "csrc", "host")


def test_the_readers_under_the_sanitizers(tmp_path):
    """tools/input_stream_sanitized.sh: tools/input_stream_check.cpp (its own main) built with AddressSanitizer +
    UndefinedBehaviorSanitizer and again with ThreadSanitizer.  CPU only, no Python in that process, nothing preloaded."""
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "input_stream_sanitized.sh")], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, TMPDIR=str(tmp_path)))
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-1500:])
    runs = re.findall(r"input_stream_check: (\d+) checks, all as the model has them", r.stdout)
    assert len(runs) == 2 and runs[0] == runs[1] and int(runs[0]) > 500, r.stdout[-500:]


def test_one_reader_and_one_loop_in_the_hosts():
    """The hosts hold no reader or read-ahead loop of their own: every std::thread of the input path is stream_batches'."""
    for name in ("train.cpp", "eval.cpp", "bam_reader.h"):
        text = open(os.path.join(HOST, name)).read()
        assert "std::thread" not in text and "last28" not in text and "pread(" not in text, name
    stream = open(os.path.join(HOST, "input_stream.h")).read()
    assert stream.count("std::thread reader(") == 1 and stream.count("bool fill(int i)") == 1
    # the error texts, verbatim
    for text in ("a line of the SAM text is longer than 64 MB", '"Error: corrupt BGZF member at file offset "',
                 '"Error: truncated BGZF member at file offset "', 'std::string("cannot open ") + kind + " file " + path'):
        assert text in stream, text
