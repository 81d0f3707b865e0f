"""bench.py's parity digests (CPU): the sorted SHA-256 and the order-free msum it prints for the
timed query must be the ones tests/golden/make_rmat_digests.py commits (oracle.digest /
oracle.msum / ora_rmat_graph_go_msum)."""
import sys
from pathlib import Path

import numpy as np

import oracle as O
from nebula_amd import synth

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import bench  # noqa: E402


def test_bench_digests_match_oracle():
    g = O.RmatGraph(14, 16, 1, threads=4)
    starts = synth.seeds(14, 16, 1, 16)
    rows, _ = g.go(starts, 2)
    shuffled = np.random.default_rng(0).permutation(rows)
    assert bench.O_digest(shuffled) == O.digest(rows)
    assert bench.msum(shuffled, chunk=1000) == O.msum(rows)
    assert bench.msum(shuffled) == g.go_msum(starts, 2)[0]


def _host_copy(dst, src, nbytes, kind):
    """stands in for hipMemcpy behind GraphSpace.L: the "device" column lives in host memory"""
    import ctypes
    assert kind == 2  # hipMemcpyDeviceToHost
    ctypes.memmove(dst, src, nbytes)
    return 0


def _dump(tmp_path, name, col, monkeypatch, cap=None):
    from types import SimpleNamespace
    if cap:
        monkeypatch.setattr(bench, "DUMP_CAP_BYTES", cap)
    col = np.ascontiguousarray(col, dtype=np.int64)
    rows = SimpleNamespace(n_rows=len(col), edges_scanned=12345, cols=[col.ctypes.data])
    sp = SimpleNamespace(L=SimpleNamespace(hipDeviceSynchronize=lambda: 0, hipMemcpy=_host_copy))
    bench.dump_go(tmp_path / name, "", sp, rows)
    return np.load(tmp_path / name / "go_dst.npy"), np.load(tmp_path / name / "go_summary.npy")


def test_dump_outputs_is_order_free_and_bounded(tmp_path, monkeypatch):
    """--dump-outputs of a GO: the same bag of rows in another order gives the same files; the
    summary holds the msum of every row; a column over the cap is sampled by vid hash, so the
    sample of a result is a subset of it chosen by value alone"""
    rng = np.random.default_rng(1)
    rows = rng.integers(-(1 << 63), (1 << 63) - 1, size=50_000)  # vids use all 64 bits
    n, s, x = bench.msum(rows)
    a, sa = _dump(tmp_path, "a", rows, monkeypatch)
    b, sb = _dump(tmp_path, "b", rng.permutation(rows), monkeypatch)
    assert a.dtype == np.float64 and np.array_equal(a, bench.split64(np.sort(rows)))
    back = (a[:, 0].astype(np.int64) << 32) | a[:, 1].astype(np.int64)
    assert np.array_equal(back, np.sort(rows))  # the halves are exact
    assert np.array_equal(a, b) and np.array_equal(sa, sb)
    assert sa.tolist() == [n, 12345, 1] + bench.limbs16(s) + bench.limbs16(x)
    # 50 000 rows x 16 B against a 64 KiB cap: modulus 32, the rows with hash % 32 == 0, sorted
    c, sc = _dump(tmp_path, "c", rows, monkeypatch, cap=64 << 10)
    d, _ = _dump(tmp_path, "d", rng.permutation(rows), monkeypatch, cap=64 << 10)
    assert sc[2] == 32 and c.nbytes <= 64 << 10 and np.array_equal(c, d)
    want = np.sort(rows[(bench.mix64(rows.astype(np.int64).view(np.uint64)) & np.uint64(31)) == 0])
    assert np.array_equal(c, bench.split64(want[:(64 << 10) // 16]))
    assert sc.tolist()[3:] == sa.tolist()[3:]  # the digest still covers every row
