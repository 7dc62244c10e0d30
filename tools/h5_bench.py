"""Load time of a large `--lowmem` HDF5 store: the GPU path (utm_h5_*: LZF decode and packing on the device) against a
host path (utm_lzf_decode_host on up to 16 threads, then numpy packing).  The store is written with tests/h5_gen.py
from a few hundred distinct compressed chunks, so that writing it stays fast.  Prints one JSON line: seconds of both
paths, the HIP-event split of the GPU path (h2d / decode / pack / d2h), and whether the outputs are equal.

--write measures the other direction, writing such a store from packed rows: the GPU writer (h5write.py with utm_h5w_*,
end to end and split by HIP events: h2d / cells / encode / d2h) against the cells built by numpy and LZF-encoded by
utm_lzf_encode_host on --threads host threads and on one thread (as liblzf runs inside h5py).  The file is not
written by the host paths; every path's stored chunks are compared.

    python tools/h5_bench.py [--rows 2000000] [--samples 2504] [--kind bool|float32] [--distinct 300] [--write]
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
from utmos_amd.h5write import H5Writer, data_chunk_rows, store_chunk  # noqa: E402


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


def packed_rows(n_rows, n_samples, kind, distinct, seed=1):
    """(packbits rows, float32 AF): n_rows rows drawn from `distinct` random blocks of 997 rows."""
    rng = np.random.default_rng(seed)
    blocks = [np.packbits(rng.random((997, n_samples)) < rng.random() * 0.1 * rng.random((997, 1)) ** 2, axis=1)
              for _ in range(distinct)]
    order = rng.integers(0, distinct, (n_rows + 996) // 997)
    rows = np.concatenate([blocks[b] for b in order])[:n_rows]
    af = (rng.integers(1, 2 * n_samples, n_rows) / (2 * n_samples)).astype(np.float32)
    return rows, af


def host_encode(rows, af, n_samples, with_af, threads):
    chunk_rows = data_chunk_rows(n_samples)
    t = time.perf_counter()

    def one(lo):
        gt = np.unpackbits(rows[lo:lo + chunk_rows], axis=1, count=n_samples)
        full = np.zeros((chunk_rows, n_samples), np.float32 if with_af else bool)
        full[:len(gt)] = gt.astype(np.float32) * af[lo:lo + chunk_rows, None] if with_af else gt
        return store_chunk(full.tobytes())

    with ThreadPoolExecutor(threads) as pool:
        chunks = list(pool.map(one, range(0, len(rows), chunk_rows)))
    return time.perf_counter() - t, chunks


def bench_write(args, tmp):
    rows, af = packed_rows(args.rows, args.samples, args.kind, args.distinct)
    with_af = args.kind == "float32"
    names = [f"S{k:06d}" for k in range(args.samples)]
    var_count = np.zeros(args.samples, np.int64)
    path = os.path.join(tmp, "w.hdf5")
    result = {}
    for attempt in range(2):                                  # the first one warms up the library and the device
        t = time.perf_counter()
        with H5Writer(path, names, with_af, "gpu") as w:
            for lo in range(0, len(rows), 1 << 18):
                w.add_rows(rows[lo:lo + (1 << 18)], af[lo:lo + (1 << 18)])
            split = w.enc.timing()
            w.finish(var_count)
        result = {"gpu_s": round(time.perf_counter() - t, 3), "gpu_ms": {k: round(v, 1) for k, v in split.items()}}
    store = H5Store(path)
    with open(path, "rb") as fh:
        stored = []
        for _row, offset, size, mask in store.data.chunks:
            fh.seek(offset)
            stored.append((fh.read(size), mask))
    host_s, host = host_encode(rows, af, args.samples, with_af, args.threads)
    one_s, one = host_encode(rows, af, args.samples, with_af, 1)
    print(json.dumps({"mode": "write", "rows": args.rows, "samples": args.samples, "kind": args.kind,
                      "chunks": len(stored), "raw_chunks": sum(m for _b, m in stored),
                      "cell_bytes": args.rows * args.samples * (4 if with_af else 1),
                      "stored_bytes": sum(len(b) for b, _m in stored), "file_bytes": os.path.getsize(path), **result,
                      "host_s": round(host_s, 3), "host_threads": args.threads, "host1_s": round(one_s, 3),
                      "speedup_vs_threads": round(host_s / result["gpu_s"], 2),
                      "speedup_vs_one": round(one_s / result["gpu_s"], 2),
                      "equal": stored == host == one}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2_000_000)
    ap.add_argument("--samples", type=int, default=2504)
    ap.add_argument("--kind", choices=["bool", "float32"], default="bool")
    ap.add_argument("--distinct", type=int, default=300)
    ap.add_argument("--threads", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--dir", default=None)
    ap.add_argument("--write", action="store_true", help="measure writing a store instead of loading one")
    args = ap.parse_args()
    if args.write:
        with tempfile.TemporaryDirectory(dir=args.dir) as tmp:
            bench_write(args, tmp)
        return
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
