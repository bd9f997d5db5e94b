"""The argument checks in front of the reference ingest and haplotype assembly kernels without a GPU
(simuscop_amd/csrc/sg_hap_check.h: sg_reference_chunk, sg_reference_commit, sg_build_haplotypes' pieces, patches,
literals and tiling, sg_haplotype_codes, the call-order refusals): the stand-alone sanitizer build of
tools/hap_check_fuzz.cpp against its byte-marking restatement, and where the checks live."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "simuscop_amd", "csrc")


def test_the_checks_under_the_sanitizers(tmp_path):
    """tools/hap_check_sanitized.sh: every clause with its legal neighbour, the values whose 64-bit sums wrap, overlap plus
    gap, shuffled lists, pieces of length 0, and 4,000 seeded random lists of at most 12 pieces on chains of at most 64
    bytes of which about half are legal (the program itself refuses a share outside 30..70 %).  CPU only."""
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "hap_check_sanitized.sh"), "4000", "99"], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, TMPDIR=str(tmp_path)))
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    assert "every verdict as the restatement has it" in r.stdout
    m = re.search(r"4000 random lists, (\d+) legal", r.stdout)
    assert m and 1200 <= int(m.group(1)) <= 2800, r.stdout


def test_the_header_reaches_no_hip_header_and_the_entry_points_hold_no_check_of_their_own():
    hdr = open(os.path.join(CSRC, "sg_hap_check.h")).read()
    assert set(re.findall(r'#include [<"]([^>"]+)[>"]', hdr)) == {"stdint.h", "algorithm", "string", "vector", "simuscop_amd.h"}
    assert not re.search(r"#include [<\"]hip", open(os.path.join(ROOT, "include", "simuscop_amd.h")).read())
    api = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "sg_api_haplotypes.cpp")).read())
    # no sum is compared against a limit in the entry points any more: the ranges are decided in the header alone
    assert not re.search(r"\+\s*[\w.>\-]+\s*>\s*(ctx->|lens\[|n_literal)", api)
    for call in ("chk::chunk(", "chk::need_image(", "chk::contig(", "chk::need_contigs(", "chk::piece(", "chk::tiling(", "chk::patch(", "chk::codes("):
        assert call in api, call
    # the message texts are the header's, one place each
    for text in ("falls outside its chain", "falls outside its contig", "falls outside the literal bytes", "runs past the end of the file",
                 "range past the end of the chain", "range outside sg_reference_begin's size"):
        assert text in hdr and text not in api, text
