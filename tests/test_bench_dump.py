"""bench.py --dump-outputs (no GPU): what `dump_outputs` writes for a pass, against a session stand-in that serves known
text the way the engine's sg_fetch_range does."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Engine:
    def __init__(self, mates):
        self.mates = mates

    def sg_fetch_range(self, ctx, mate, off, n, dst):
        text = self.mates[mate]
        assert 0 <= off and off + n <= len(text), (mate, off, n, len(text))
        C.memmove(dst.value, text[off:off + n], n)
        return 0


class _Session:
    """result(), host_alloc / host_free, _sg and eng.sg_fetch_range: the part of simuscop_amd.Session the dump uses."""

    def __init__(self, mates, pairs):
        self.eng = _Engine(mates)
        self.ctx = None
        self.pairs = pairs
        self.bufs = {}

    def result(self):
        return len(self.eng.mates[0]), len(self.eng.mates[1]), self.pairs

    def host_alloc(self, n):
        b = C.create_string_buffer(n)
        self.bufs[C.addressof(b)] = b
        return C.addressof(b)

    def host_free(self, p):
        del self.bufs[p]

    def _sg(self, rc, what):
        assert rc == 0, what


def _run(tmp_path, mates, pairs=7):
    sys.path.insert(0, ROOT)
    import bench
    sess = _Session(mates, pairs)
    d = str(tmp_path / "dump")
    bench.dump_outputs(sess, d)
    assert not sess.bufs
    return bench, d


def test_dump_of_a_pass_larger_than_one_copy(tmp_path):
    rng = np.random.default_rng(5)
    n1, n2 = (1 << 26) + 3 * (1 << 16) + 777, (1 << 26) - 5
    mates = [rng.integers(33, 127, n, dtype=np.uint8).tobytes() for n in (n1, n2)]
    bench, d = _run(tmp_path, mates)
    files = sorted(os.listdir(d))
    assert files == ["counts.npy", "mate1_block_sums.npy", "mate1_text_sample.npy", "mate2_block_sums.npy", "mate2_text_sample.npy"]
    assert sum(os.path.getsize(os.path.join(d, f)) for f in files) <= 64 << 20
    assert np.load(os.path.join(d, "counts.npy")).tolist() == [n1, n2, 7]
    for m, text in enumerate(mates, 1):
        arr = np.frombuffer(text, dtype=np.uint8)
        sums = np.load(os.path.join(d, f"mate{m}_block_sums.npy"))
        assert sums.dtype == np.float64
        B = bench.DUMP_SUM_BLOCK
        assert sums.tolist() == [float(arr[i:i + B].sum()) for i in range(0, len(arr), B)]
        sample = np.load(os.path.join(d, f"mate{m}_text_sample.npy"))
        assert sample.dtype == np.float32 and sample.shape == (bench.DUMP_SAMPLE_CHUNKS, bench.DUMP_SAMPLE_BYTES)
        S = bench.DUMP_SAMPLE_BYTES
        assert np.array_equal(sample[0], arr[:S]) and np.array_equal(sample[1], arr[-S:])
        # every chunk is a stretch of the text
        starts = {text.find(sample[i].astype(np.uint8).tobytes()) for i in range(len(sample))}
        assert -1 not in starts


def test_dump_is_the_same_for_the_same_pass_and_single_end_has_no_mate_2(tmp_path):
    text = bytes(np.random.default_rng(9).integers(33, 127, 100_000, dtype=np.uint8))
    _, d1 = _run(tmp_path / "a", [text, b""])
    _, d2 = _run(tmp_path / "b", [text, b""])
    assert sorted(os.listdir(d1)) == ["counts.npy", "mate1_block_sums.npy", "mate1_text_sample.npy"]
    for f in os.listdir(d1):
        assert np.array_equal(np.load(os.path.join(d1, f)), np.load(os.path.join(d2, f))), f
