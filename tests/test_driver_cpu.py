"""The simuReads driver's parts that need no GPU: the chunk pump of the FASTQ sink (pump_chunks, host/fastq_sink.h) with
64-byte chunks -- the product's are 64 MB, which keeps every chunk boundary out of the quick tests' reach -- and the two
cuts of a batch (host/batch_cut.h) against a brute-force restatement, in a stand-alone program under the sanitizers; and
where the driver's subjects live in the sources."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "simuscop_amd", "csrc", "host")


def test_the_pump_and_the_cuts_under_the_sanitizers(tmp_path):
    """tools/driver_sanitized.sh: tools/driver_check.cpp (its own main) built with AddressSanitizer +
    UndefinedBehaviorSanitizer and again with ThreadSanitizer.  CPU only, no Python in that process, nothing preloaded."""
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "driver_sanitized.sh")], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, TMPDIR=str(tmp_path)))
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-1500:])
    runs = re.findall(r"driver_check: (\d+) checks, all as the model has them", r.stdout)
    assert len(runs) == 2 and runs[0] == runs[1] and int(runs[0]) > 10000, r.stdout[-500:]


def test_each_subject_of_the_driver_in_its_own_file():
    """Threads, engine calls of the sinks and the planner, and the files' error texts: where they are and where not."""
    text = {n: open(os.path.join(HOST, n)).read() for n in sorted(os.listdir(HOST)) if n.endswith((".h", ".cpp"))}
    # the output side's threads are the FASTQ sink's; the others are input and planning: the reference ingest's readers
    # (fasta.cpp, reader_pool.h), the read-ahead loop of seqToProfile and truthEval (input_stream.h), the haplotype pool
    # of the planner (read_plan.cpp) and the profile loader of Driver::open (simulate.cpp)
    threads = {n for n, t in text.items() if "std::thread" in t}
    assert threads == {"fastq_sink.h", "fastq_sink.cpp", "fasta.cpp", "reader_pool.h", "input_stream.h", "read_plan.cpp", "simulate.cpp"}, threads
    assert text["simulate.cpp"].count("std::thread") == 2 and "std::thread prof_thread(" in text["simulate.cpp"]
    for call in ("sg_outputs_fetch", "sg_truth_bam", "sg_bamsort_pass", "sg_plan_windows", "sg_window_weights"):
        assert call not in text["simulate.cpp"], call
    assert "sg_outputs_fetch(" in text["fastq_sink.cpp"] and "sg_" not in text["batch_cut.h"]
    for call in ("sg_truth_bam(", "sg_truth_bam_tags(", "sg_bamsort_pass("):
        assert call in text["truth_bam.cpp"], call
    for call in ("sg_plan_windows(", "sg_window_weights("):
        assert call in text["read_plan.cpp"], call
    # the error texts, verbatim
    for said, where in (("can not open fastq file to save results", "fastq_sink.cpp"), ("short write to fastq file", "fastq_sink.cpp"),
                        ("can not open BAM file to save the true alignments", "truth_bam.cpp"),
                        ("short write to the truth BAM file", "truth_bam.cpp")):
        assert said in text[where], said
