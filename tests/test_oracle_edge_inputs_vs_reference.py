"""Degenerate configurations (tests/edge_inputs.py): oracle(mt) against the UNMODIFIED reference binary -- same files byte
for byte where the reference runs, a refusal where it refuses (or never returns).  The binary runs here and now where
oracle/_ref/simuReads is built; elsewhere its recorded runs stand in (tests/ref_runs.py)."""
import os

import pytest

import cases
import edge_inputs
import ref_runs


@pytest.mark.parametrize("name", edge_inputs.NAMES)
def test_oracle_mt_equals_reference_on_degenerate_configuration(name, oracle_lib, tmp_path):
    cfg = edge_inputs.build(name, str(tmp_path))
    out = os.path.join(str(tmp_path), "out")
    # (these cases take the reference seconds; a copy-number gain on a haploid genome spins for ever, Segment.cpp:188-197)
    ref_rc, want = ref_runs.run(f"edge/{name}", cfg, out, timeout=40)
    rc = oracle_lib.orc_simulate(cfg.encode(), 0, cases.FAKE_SEC, cases.FAKE_NSEC, b"", 1)
    if ref_rc != 0:
        assert rc != 0, "the oracle accepted what the reference refused"
        return
    assert rc == 0, oracle_lib.orc_last_error().decode()
    assert ref_runs.md5s(out) == want
