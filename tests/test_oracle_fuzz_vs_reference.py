"""Random configurations against the UNMODIFIED reference binary: oracle(mt) must write the binary's bytes.

The committed golden sums pin named cases; this test draws configurations from the GPU fuzz generator
(tests/test_gpu_fuzz.py: contig counts and sizes, profile, layout, coverage, insert size, ploidy, variants, SNPs, N islands,
BED targets incl. overlapping / nested / unsorted ones, mixtures, derived read lengths and indel rates) and runs both
programs on each, here and now where oracle/_ref/simuReads is built (`make -C oracle ref`); elsewhere the binary's recorded
runs of the default seeds stand in (tests/ref_runs.py).  SIMU_REF_FUZZ_SEEDS=a-b widens it (binary needed): seeds 101-148,
201-260 and 1001-1030 -- all 138 seeds of the GPU fuzz -- and 300-999, 1031-2710 were run this way in round 3: 2,517 byte-identical (592 -- one target
inside an N run: a genome without weighted length -- after the oracle stopped refusing what the binary samples nothing
from), one (1021: a copy-number gain on a haploid genome) is the documented case the reference never returns from."""
import os
import random

import pytest

import cases
import ref_runs
import test_gpu_fuzz as fz


def _seeds():
    env = os.environ.get("SIMU_REF_FUZZ_SEEDS")
    if env:
        a, b = env.split("-")
        return list(range(int(a), int(b) + 1))
    return [103, 117, 131, 205, 219, 233, 247, 1003, 1013, 1016, 1023, 1028]


@pytest.mark.parametrize("seed", _seeds())
def test_oracle_mt_equals_reference_on_random_configuration(seed, oracle_lib, tmp_path):
    rng = random.Random(seed)
    cfg = fz._make(rng, str(tmp_path), extended=seed >= 200, tight_targets=seed >= 1000)
    out = os.path.join(str(tmp_path), "out")
    ref_rc, want = ref_runs.run(f"fuzz/{seed}", cfg, out, timeout=120)
    rc = oracle_lib.orc_simulate(cfg.encode(), 0, cases.FAKE_SEC, cases.FAKE_NSEC, b"", 1)
    if ref_rc is None:
        # the one configuration class the reference never returns from (Segment.cpp:188-197): the oracle refuses it
        assert rc != 0
        return
    if ref_rc != 0:
        assert rc != 0, "the oracle accepted what the reference refused"
        return
    assert rc == 0, oracle_lib.orc_last_error().decode()
    assert ref_runs.md5s(out) == want and want
