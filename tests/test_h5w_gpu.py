"""Writing the reference's `--lowmem` HDF5 store on the GPU (utm_h5w_*, csrc/lzf_enc.hip.h, utmos_amd/h5write.py):
`select --lowmem X.hdf5` against the reference's files byte for byte (repo_utils/utmos_ssshtests.sh:197-223) and
against the answer files, the written files read back by the reference's reuse cases, the device's stored chunks
against utm_lzf_encode_host on generated matrices, and the context's slot rules."""
import ctypes
import os

import numpy as np
import pytest

import oracle_util as ou
from test_h5_gpu import REFERENCE_CASES, gpu_rows, run_cli
from test_h5_host import TINY, TINY_AF
from test_h5w_host import check_read_back, write

pytestmark = pytest.mark.gpu
CASES = ou.golden_cases()
JL2 = os.path.join(ou.GOLD, "jl", "chunk2.jl")


def npz(name):
    return os.path.join(ou.GOLD, f"{name}.npz")


@pytest.mark.parametrize("source", ["npz", "jl"])
def test_select_writes_the_reference_store(source, tmp_path):
    store, out = str(tmp_path / "OUT.hdf5"), str(tmp_path / "out.txt")
    run_cli(["--maxmem", "0", "--lowmem", store, "-o", out, npz("chunk2") if source == "npz" else JL2])
    assert open(out).read() == ou.golden_text(CASES["select_first"])
    assert open(store, "rb").read() == open(TINY, "rb").read()
    for name in ("p1_lm", "p2_lm"):
        argv, golden = REFERENCE_CASES[name]
        reuse = str(tmp_path / f"{name}.txt")
        run_cli([store if a == TINY else a for a in argv] + ["-o", reuse])
        assert open(reuse).read() == ou.golden_text(CASES[golden])


def test_select_writes_the_reference_af_store(tmp_path):
    store, out = str(tmp_path / "OUT.af.hdf5"), str(tmp_path / "out.txt")
    run_cli(["--maxmem", "0", "-c", "20", "--af", "--lowmem", store, "-o", out, npz("chunk0"), npz("chunk1")])
    assert open(out).read() == ou.golden_text(CASES["select_af_h5"])
    assert open(store, "rb").read() == open(TINY_AF, "rb").read()
    for name in ("af_p1_lm", "af_p2_lm"):
        argv, golden = REFERENCE_CASES[name]
        reuse = str(tmp_path / f"{name}.txt")
        run_cli([store if a == TINY_AF else a for a in argv] + ["-o", reuse])
        assert open(reuse).read() == ou.golden_text(CASES[golden])


@pytest.mark.parametrize("af", [False, True])
def test_several_dumps_give_the_utm_paths_selection(af, tmp_path):
    inputs = [npz("chunk0"), npz("chunk1"), npz("chunk2")]
    flags = ["--maxmem", "0", "--buffer", "256", "-c", "30"] + (["--af"] if af else [])
    outs = []
    for suffix in (".hdf5", ".utm"):
        out = str(tmp_path / f"out{suffix}.txt")
        run_cli(flags + ["--lowmem", str(tmp_path / f"s{suffix}"), "-o", out] + inputs)
        outs.append(open(out).read())
    assert outs[0] == outs[1]
    reuse = str(tmp_path / "reuse.txt")
    run_cli(flags + ["-o", reuse, str(tmp_path / "s.hdf5")])
    assert open(reuse).read() == outs[0]


def generated(kind, n_rows, n_samples, seed):
    rng = np.random.default_rng(seed)
    dens = rng.random((n_rows, 1)) * 0.03
    gt = rng.random((n_rows, n_samples)) < dens
    gt[::7] = gt[3]                                          # repeated rows: matches far back
    rows = np.packbits(gt, axis=1)
    af = (rng.integers(1, 2 * n_samples, n_rows) / (2 * n_samples)).astype(np.float32)
    return rows, af, np.array([f"S{k:06d}" for k in range(n_samples)]), kind == "float32"


@pytest.mark.parametrize("kind, n_rows, n_samples, max_chunks", [
    ("bool", 200_003, 2504, None), ("float32", 200_003, 2504, None),
    ("bool", 20_000, 2504, 1), ("float32", 20_000, 2504, 3),
    ("float32", 5, 250_007, None),                           # one-row chunks
])
def test_device_chunks_equal_the_host_encoder(kind, n_rows, n_samples, max_chunks, tmp_path):
    rows, af, samples, with_af = generated(kind, n_rows, n_samples, n_rows + n_samples)
    gpu = write(tmp_path / "g.hdf5", rows, af, samples, with_af, "gpu", piece=50_000, max_chunks=max_chunks)
    host = write(tmp_path / "h.hdf5", rows, af, samples, with_af, "host", piece=50_000)
    assert open(gpu, "rb").read() == open(host, "rb").read()
    if n_rows < 100_000:
        check_read_back(gpu, rows, af, samples, with_af)
    g_rows, g_af = gpu_rows(gpu)                             # and the device decoder reads it back
    assert np.array_equal(g_rows, rows)
    if with_af:
        assert g_af.tobytes() == np.where(rows.any(axis=1), af, np.float32(0)).tobytes()


def test_incompressible_chunks_are_stored_raw(tmp_path):
    from utmos_amd.h5store import H5Store
    n = 250_000 + 17                                         # one sample: chunks of 250,000 float32 cells
    rows = np.packbits(np.ones((n, 1), bool), axis=1)
    af = np.random.default_rng(4).random(n).astype(np.float32)
    gpu = write(tmp_path / "g.hdf5", rows, af, np.array(["A"]), True, "gpu", piece=100_000)
    host = write(tmp_path / "h.hdf5", rows, af, np.array(["A"]), True, "host", piece=100_000)
    assert open(gpu, "rb").read() == open(host, "rb").read()
    masks = [c[3] for c in H5Store(gpu).data.chunks]
    assert masks == [1, 0]
    g_rows, g_af = gpu_rows(gpu)
    assert np.array_equal(g_rows, rows) and g_af.tobytes() == af.tobytes()


def test_slot_errors_leave_the_context_usable():
    from utmos_amd import _native as nat
    from utmos_amd.h5write import GpuChunkEncoder
    lib = nat.lib()
    rows, af, _, _ = generated("float32", 400, 2504, 1)
    enc = GpuChunkEncoder(99, 2504, 4, 0, max_chunks=2)
    try:
        out, n_bytes, n = ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_uint32()
        sizes, masks = np.zeros(2, np.uint32), np.zeros(2, np.uint32)
        assert lib.utm_h5w_fetch(enc.h, ctypes.byref(out), ctypes.byref(n_bytes), sizes.ctypes.data,
                                 masks.ctypes.data, ctypes.byref(n)) == -4          # nothing queued
        assert lib.utm_h5w_encode(enc.h, rows.ctypes.data, None, 99) != 0           # float32 without AF
        assert lib.utm_h5w_encode(enc.h, rows.ctypes.data, af.ctypes.data, 199) != 0  # more than two chunks
        assert lib.utm_h5w_encode(enc.h, rows.ctypes.data, af.ctypes.data, 0) != 0
        enc.submit(rows[:150], af[:150])
        enc.submit(rows[150:300], af[150:300])
        with pytest.raises(nat.NativeError, match="both slots") as err:
            enc.submit(rows[:10], af[:10])
        assert err.value.code == -4
        first = enc.results(final=True)
        assert [len(b[1]) for b in first] == [2, 2]
        enc.submit(rows[:150], af[:150])                                            # into a freed slot
        again = enc.results(final=True)
        assert again[0] == first[0]
        ms = enc.timing()
        assert all(v >= 0 for v in ms.values()) and ms["encode"] > 0
    finally:
        enc.close()
