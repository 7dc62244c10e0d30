"""Load time of a large `--lowmem` HDF5 store: the GPU path (utm_h5_*: LZF decode and packing on the device) against a
host path (utm_lzf_decode_host on up to 16 threads, then numpy packing).  The store is written with tests/h5_gen.py
from a few hundred distinct compressed chunks, so that writing it stays fast.  Prints one JSON line: seconds of both
paths, the HIP-event split of the GPU path (h2d / decode / pack / d2h), and whether the outputs are equal.

    python tools/h5_bench.py [--rows 2000000] [--samples 2504] [--kind bool|float32] [--distinct 300]
"""
import argparse
import json
import os
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import h5_gen  # noqa: E402
from utmos_amd.h5store import ChunkDecoder, H5Store, lzf_decode, pack_rows  # noqa: E402


def write(path, n_rows, n_samples, kind, distinct, seed=1):
    rng = np.random.default_rng(seed)
    chunk_rows = h5_gen.chunk_rows_for(n_samples)
    n_chunks = (n_rows + chunk_rows - 1) // chunk_rows
    blobs = []
    for _ in range(distinct):
        gt = rng.random((chunk_rows, n_samples)) < rng.random() * 0.1 * rng.random((chunk_rows, 1)) ** 2
        if kind == "float32":
            af = (rng.integers(1, 2 * n_samples, chunk_rows) / (2 * n_samples)).astype(np.float32)
            cells = np.where(gt, af[:, None], np.float32(0)).astype(np.float32)
        else:
            cells = gt
        blobs.append(h5_gen.encode_chunks(cells, chunk_rows)[0][1:])
    order = rng.integers(0, distinct, n_chunks)
    chunks = [(k * chunk_rows,) + blobs[b] for k, b in enumerate(order)]
    h5_gen.write_store(path, chunks=chunks, shape=(n_rows, n_samples), chunk_rows=chunk_rows,
                       dtype=np.bool_ if kind == "bool" else np.float32)


def gpu_load(path):
    t = time.perf_counter()
    with ChunkDecoder(H5Store(path), 0) as dec:
        parts = list(dec)
        split = dec.timing()
    rows = np.concatenate([p[1] for p in parts])
    af = None if parts[0][2] is None else np.concatenate([p[2] for p in parts])
    return time.perf_counter() - t, split, rows, af


def host_load(path, threads=16):
    t = time.perf_counter()
    store = H5Store(path)
    ds = store.data

    def one(chunk):
        row, offset, size, mask = chunk
        with open(path, "rb") as fh:
            fh.seek(offset)
            blob = fh.read(size)
        raw = blob if mask & 1 else lzf_decode(blob, ds.chunk_bytes)
        cells = np.frombuffer(raw, ds.dtype).reshape(ds.chunk_shape)[:min(ds.chunk_rows, ds.shape[0] - row)]
        return pack_rows(cells)

    with ThreadPoolExecutor(threads) as pool:
        parts = list(pool.map(one, ds.chunks))
    rows = np.concatenate([p[0] for p in parts])
    af = None if parts[0][1] is None else np.concatenate([p[1] for p in parts])
    return time.perf_counter() - t, rows, af


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2_000_000)
    ap.add_argument("--samples", type=int, default=2504)
    ap.add_argument("--kind", choices=["bool", "float32"], default="bool")
    ap.add_argument("--distinct", type=int, default=300)
    ap.add_argument("--threads", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--dir", default=None)
    args = ap.parse_args()
    with tempfile.TemporaryDirectory(dir=args.dir) as tmp:
        path = os.path.join(tmp, "bench.hdf5")
        t = time.perf_counter()
        write(path, args.rows, args.samples, args.kind, args.distinct)
        write_s = time.perf_counter() - t
        gpu_load(path)                                        # warm-up: library load, first context, page cache
        gpu_s, split, g_rows, g_af = gpu_load(path)
        host_s, h_rows, h_af = host_load(path, args.threads)
        equal = bool(np.array_equal(g_rows, h_rows) and ((g_af is None and h_af is None) or
                                                         (g_af is not None and g_af.tobytes() == h_af.tobytes())))
        print(json.dumps({"rows": args.rows, "samples": args.samples, "kind": args.kind,
                          "file_bytes": os.path.getsize(path), "cell_bytes": args.rows * args.samples *
                          (1 if args.kind == "bool" else 4), "write_s": round(write_s, 2),
                          "gpu_s": round(gpu_s, 3), "gpu_ms": {k: round(v, 1) for k, v in split.items()},
                          "host_s": round(host_s, 3), "host_threads": args.threads,
                          "speedup": round(host_s / gpu_s, 2), "equal": equal}))


if __name__ == "__main__":
    main()
