"""VCF ingest benchmark: the CPU reader (utmos_amd/vcfio.read_vcf) against the GPU reader (utmos_amd/vcfgpu.py) on one
seeded synthetic call set, uncompressed and BGZF, end to end in the same process, with the GPU reader's phase split.

    python tools/vcf_bench.py --out DIR [--records 200000] [--samples 2504] [--seed 1] [--device 0] [--inflate both] [--bcf]

Writes DIR/synth.vcf and DIR/synth.vcf.gz (BGZF, zlib level 1: inflate speed barely depends on the level), prints one
JSON line and writes it to DIR/vcf_bench.json.  The call set: FORMAT GT, `a|b` / `a/b` diploid calls, about 10 % of
records multi-allelic (2-3 alt alleles), 1 % missing alleles.  Phases (seconds unless named _ms):
  fill_s      host: reading (plain) or inflating (BGZF, thread pool) the text into the pinned staging; with BGZF
              inflated on the GPU, reading the compressed members into the staging
  h2d_ms, kernel_ms, d2h_ms   HIP-event time of the copies and of the four parse kernels, summed over the batches
  inflate_ms  HIP-event time of the BGZF inflate kernels (GPU inflation only)
BGZF is read with GPU inflation (gpu_bgzf) and with host inflation (gpu_bgzf_host_inflate); --inflate picks one.
--bcf writes the same call set as BCF too (DIR/synth.raw.bcf the bare stream, DIR/synth.bcf in BGZF; GT as int8 x 2) and
reads it the same three ways (gpu_bcf_raw, gpu_bcf_bgzf, gpu_bcf_bgzf_host_inflate); every result must equal the plain
VCF's.  kernel_ms = find_ms + parse_ms (HIP events around each): for BCF find_ms is k_bcf_chain and parse_ms is
k_bcf_parse; for VCF find_ms is k_vcf_nl_count + k_vcf_nl_scan and parse_ms is k_vcf_nl_write + k_vcf_parse.
  total_s     the whole call, header to the assembled arrays
The write phase (skip with --skip-write) writes the call set's `convert` part file (.jl, the GT/AF/samples/stats dict)
from the GPU reader's result: joblib.dump(compress=5) (convert's host path), the same pickle deflated in independent
64 KiB segments by `min(16, cpus)` host threads (zlib.compressobj per segment, level 5), and GpuZlibWriter at levels
1 / 5 / 9 (seconds, file bytes, and the writer's HIP-event split: h2d, kernels, parse (part of kernels), d2h).  Every
file is read back and checked.  `convert` end to end (BGZF input, .jl output at -c 5) is timed with --deflate host and
--deflate gpu.  --write-only skips the reader comparisons.
Kernel time for a text GB/s figure is best taken from a `rocprofv3 --kernel-trace --stats` run of this tool; stream_gbps
is the streaming-read calibration of this GPU (utm_stream_calibration) to hold it against.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synth_blocks(seed, n_rec, n_samp, block=5000):
    """Yields the call set `block` records at a time: (first record, n_alt per record, cells (nb, n_samp, 4) as the VCF
    characters `a`, separator, `b`, tab or newline)."""
    rng = np.random.default_rng(seed)
    for b0 in range(0, n_rec, block):
        nb = min(block, n_rec - b0)
        n_alt = np.where(rng.random(nb) < 0.1, rng.integers(2, 4, nb), 1)
        af = rng.beta(0.3, 3.0, nb)[:, None]
        cells = np.empty((nb, n_samp, 4), np.uint8)
        for k in (0, 2):
            carrier = rng.random((nb, n_samp)) < af
            allele = np.where(carrier, rng.integers(1, n_alt[:, None] + 1, (nb, n_samp)), 0)
            ch = (allele + 48).astype(np.uint8)
            ch[rng.random((nb, n_samp)) < 0.01] = ord(".")
            cells[:, :, k] = ch
        cells[:, :, 1] = np.where(rng.random((nb, n_samp)) < 0.9, ord("|"), ord("/"))
        cells[:, :, 3] = ord("\t")
        cells[:, -1, 3] = ord("\n")
        yield b0, n_alt, cells


def header_text(n_samp, bcf=False):
    meta = "##fileformat=VCFv4.2\n##source=vcf_bench\n"
    if bcf:   # the lines a BCF header needs: the dictionary (PASS = 0, GT = 1) and the contig
        meta += '##FILTER=<ID=PASS,Description="All filters passed">\n##contig=<ID=chr1>\n##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">\n'
    return (meta + "\t".join(["#CHROM", "POS", "ID", "REF", "ALT", "QUAL", "FILTER", "INFO", "FORMAT"] + [f"HG{i:05d}" for i in range(n_samp)]) + "\n").encode()


ALTS = {1: "C", 2: "C,G", 3: "C,G,T"}


def vcf_piece(b0, n_alt, cells):
    parts = []
    for i in range(len(n_alt)):
        parts.append(f"chr1\t{1000 + b0 + i}\t.\tA\t{ALTS[int(n_alt[i])]}\t.\tPASS\t.\tGT\t".encode())
        parts.append(cells[i].tobytes())
    return b"".join(parts)


def bcf_piece(b0, n_alt, cells):
    """The same records as BCF: GT as int8 x 2 per sample, (allele + 1) << 1 | phased, `.` = 0."""
    import struct
    n_samp = cells.shape[1]
    al = cells[:, :, (0, 2)].astype(np.int16) - 48
    gt = np.where(al < 0, 0, (al + 1) << 1).astype(np.uint8)
    gt[:, :, 1] |= (cells[:, :, 1] == ord("|")).astype(np.uint8)
    parts = []
    for i in range(len(n_alt)):
        k = int(n_alt[i])
        shared = struct.pack("<iiiIII", 0, 999 + b0 + i, 1, 0x7F800001, (1 + k) << 16, 1 << 24 | n_samp)
        shared += b"\x07\x17A" + b"".join(b"\x17" + a.encode() for a in ALTS[k].split(",")) + b"\x11\x00"
        parts.append(struct.pack("<II", len(shared), 3 + 2 * n_samp) + shared + b"\x11\x01\x21")
        parts.append(gt[i].tobytes())
    return b"".join(parts)


def synth_text(seed, n_rec, n_samp, block=5000):
    """Yields the VCF text in pieces: header first, then `block` records at a time."""
    yield header_text(n_samp)
    for b0, n_alt, cells in synth_blocks(seed, n_rec, n_samp, block):
        yield vcf_piece(b0, n_alt, cells)


def write_inputs(out, seed, n_rec, n_samp, bcf=False):
    """-> paths {plain, bgzf[, bcf_raw, bcf_bgzf]} of the one call set, seconds."""
    import struct
    from utmos_amd.vcfgpu import bgzf_compress
    paths = {"plain": os.path.join(out, "synth.vcf"), "bgzf": os.path.join(out, "synth.vcf.gz")}
    if bcf:
        paths.update(bcf_raw=os.path.join(out, "synth.raw.bcf"), bcf_bgzf=os.path.join(out, "synth.bcf"))
    t0 = time.perf_counter()
    files = {k: open(p, "wb") for k, p in paths.items()}
    try:
        def put(text, stream):
            files["plain"].write(text)
            files["bgzf"].write(bgzf_compress(text, level=1)[:-28])   # (one end-of-file member, at the end)
            if bcf:
                files["bcf_raw"].write(stream)
                files["bcf_bgzf"].write(bgzf_compress(stream, level=1)[:-28])
        head = header_text(n_samp, bcf=True) + b"\0" if bcf else b""
        put(header_text(n_samp), b"BCF\x02\x02" + struct.pack("<I", len(head)) + head)
        for b0, n_alt, cells in synth_blocks(seed, n_rec, n_samp):
            put(vcf_piece(b0, n_alt, cells), bcf_piece(b0, n_alt, cells) if bcf else b"")
        for k in ("bgzf", "bcf_bgzf")[:2 if bcf else 1]:
            files[k].write(bgzf_compress(b"", level=1))
    finally:
        for fh in files.values():
            fh.close()
    return paths, time.perf_counter() - t0


def inflate_only(path, threads):
    """Seconds to inflate the whole BGZF file into a 64 MiB buffer, nothing else."""
    from utmos_amd.vcfgpu import open_source
    buf = np.empty(64 << 20, np.uint8)
    t0 = time.perf_counter()
    src = open_source(path, threads)
    n = 0
    try:
        while True:
            k = src.fill(memoryview(buf))
            if not k:
                break
            n += k
    finally:
        src.close()
    return time.perf_counter() - t0, n


def segments_host(raw, level, threads):
    """raw -> a zlib stream of independent 64 KiB segments deflated by a thread pool (zlib releases the GIL)."""
    import zlib
    from concurrent.futures import ThreadPoolExecutor
    seg = 1 << 16
    offs = list(range(0, len(raw), seg)) or [0]
    view = memoryview(raw)

    def one(off):
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        body = c.compress(view[off:off + seg])
        return body + (c.flush() if off == offs[-1] else c.flush(zlib.Z_SYNC_FLUSH))
    with ThreadPoolExecutor(threads) as pool:
        parts = list(pool.map(one, offs))
    from utmos_amd.zwrite import zlib_header
    return zlib_header(level) + b"".join(parts) + zlib.adler32(raw).to_bytes(4, "big")


def write_phase(args, bgz, res):
    """The .jl write: host joblib level 5, host threads on independent segments, the GPU writer at 1 / 5 / 9."""
    import io
    import joblib
    from utmos_amd import convert
    from utmos_amd.vcfgpu import inflate_threads
    from utmos_amd.zwrite import GpuZlibWriter
    data = convert.convert(bgz, device=args.device)
    data = dict(data, samples=np.asarray(data["samples"]).astype(object))
    out = {}

    def check(path):
        got = joblib.load(path)
        assert (got["GT"] == data["GT"]).all() and (got["AF"] == data["AF"]).all() and got["stats"] == data["stats"]

    path = os.path.join(args.out, "host5.jl")
    t0 = time.perf_counter()
    joblib.dump(data, path, compress=5)
    out["host_joblib_5"] = {"s": round(time.perf_counter() - t0, 3), "bytes": os.path.getsize(path)}
    check(path)
    t0 = time.perf_counter()
    buf = io.BytesIO()
    joblib.dump(data, buf, compress=0)
    raw = buf.getvalue()
    out["pickle_bytes"] = len(raw)
    out["pickle_s"] = round(time.perf_counter() - t0, 3)
    threads = inflate_threads()
    path = os.path.join(args.out, "threads5.jl")
    t0 = time.perf_counter()
    with open(path, "wb") as fh:
        fh.write(segments_host(raw, 5, threads))
    out[f"host_{threads}_threads_segments_5"] = {"s": round(time.perf_counter() - t0, 3) + out["pickle_s"],
                                                "bytes": os.path.getsize(path)}
    check(path)
    del raw, buf
    with GpuZlibWriter(io.BytesIO(), 5, args.device) as w:  # warm-up: code objects, pinned buffers
        w.write(b"warm-up" * 100_000)
    for level in (1, 5, 9):
        path = os.path.join(args.out, f"gpu{level}.jl")
        t0 = time.perf_counter()
        with GpuZlibWriter(path, level, args.device) as w:
            joblib.dump(data, w, compress=0)
        s = time.perf_counter() - t0
        out[f"gpu_{level}"] = {"s": round(s, 3), "bytes": os.path.getsize(path),
                               **{k + "_ms": round(v, 2) for k, v in w.final_timing.items()}}
        check(path)
    for mode in ("host", "gpu"):
        path = os.path.join(args.out, f"convert_{mode}.jl")
        t0 = time.perf_counter()
        part = convert.convert(bgz, device=args.device)
        convert.write(part, path, 5, deflate=mode, device=args.device)
        out[f"convert_bgzf_to_jl_{mode}_s"] = round(time.perf_counter() - t0, 3)
        check(path)
    res["write"] = out


def same(a, b):
    return (a["GT"].shape == b["GT"].shape and bool((a["GT"] == b["GT"]).all())
            and bool((a["AF"].view(np.int64) == b["AF"].view(np.int64)).all())
            and [str(s) for s in a["samples"]] == [str(s) for s in b["samples"]])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", required=True)
    ap.add_argument("--records", type=int, default=200_000)
    ap.add_argument("--samples", type=int, default=2504)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--skip-cpu", action="store_true", help="GPU reader only (e.g. under a profiler)")
    ap.add_argument("--skip-write", action="store_true", help="no write phase")
    ap.add_argument("--write-only", action="store_true", help="the write phase alone (after one GPU read)")
    ap.add_argument("--bcf", action="store_true",
                    help="also write the call set as BCF (bare stream and BGZF) and read it through the GPU reader")
    ap.add_argument("--inflate", choices=["both", "gpu", "host"], default="both",
                    help="BGZF through the GPU reader with GPU inflation, host inflation, or both [both]")
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    from utmos_amd import device, vcfgpu, vcfio

    paths, gen_s = write_inputs(args.out, args.seed, args.records, args.samples, args.bcf)
    plain, bgz = paths["plain"], paths["bgzf"]
    text_bytes = os.path.getsize(plain)
    res = {"records": args.records, "samples": args.samples, "text_bytes": text_bytes, "bgzf_bytes": os.path.getsize(bgz),
           "generate_s": round(gen_s, 2), "inflate_threads": vcfgpu.inflate_threads()}

    if args.write_only:
        write_phase(args, bgz, res)
        line = json.dumps(res)
        print(line)
        with open(os.path.join(args.out, "vcf_bench.json"), "w") as fh:
            fh.write(line + "\n")
        return
    # inflate alone: one thread, then the pool the reader uses
    for label, threads in (("1", 1), ("pool", vcfgpu.inflate_threads())):
        s, n = inflate_only(bgz, threads)
        assert n == text_bytes
        res[f"inflate_{label}_thread_s" if label == "1" else "inflate_pool_s"] = round(s, 3)

    runs = [("plain", plain, "auto")]
    if args.inflate in ("both", "gpu"):
        runs.append(("bgzf", bgz, "gpu"))
    if args.inflate in ("both", "host"):
        runs.append(("bgzf_host_inflate", bgz, "host"))
    gpu = {}
    for form, path, inflate in runs:
        with vcfgpu.GpuVcfReader(device=args.device, inflate=inflate) as reader:
            reader.read(os.path.join(ROOT, "tests", "golden", "vcf", "chunk0.vcf.gz"))  # warm-up: code objects, context
            gpu[form] = reader.read(path)
            res[f"gpu_{form}"] = {k: round(v, 3) for k, v in {**reader.timing, **reader.kernel_timing}.items()}
        assert same(gpu["plain"], gpu[form])
    if args.bcf:   # the same calls as BCF: bare stream, BGZF inflated on the GPU, BGZF inflated on the host
        res["bcf_bytes"], res["bcf_bgzf_bytes"] = os.path.getsize(paths["bcf_raw"]), os.path.getsize(paths["bcf_bgzf"])
        for form, path, inflate in (("bcf_raw", paths["bcf_raw"], "auto"), ("bcf_bgzf", paths["bcf_bgzf"], "gpu"),
                                    ("bcf_bgzf_host_inflate", paths["bcf_bgzf"], "host")):
            with vcfgpu.GpuVcfReader(device=args.device, inflate=inflate) as reader:
                reader.read(os.path.join(ROOT, "tests", "golden", "vcf", "chunk0.vcf.gz"))  # warm-up, as above
                got = reader.read(path)
                res[f"gpu_{form}"] = {k: round(v, 3) for k, v in {**reader.timing, **reader.kernel_timing}.items()}
            assert same(gpu["plain"], got)
            del got
        for a, b in (("bcf_bgzf", "bgzf"), ("bcf_bgzf_host_inflate", "bgzf_host_inflate"), ("bcf_raw", "plain")):
            if f"gpu_{b}" in res:
                res[f"speedup_{a}_over_vcf_{b}"] = round(res[f"gpu_{b}"]["total_s"] / res[f"gpu_{a}"]["total_s"], 2)
    if "bgzf" not in gpu:
        gpu["bgzf"] = gpu["bgzf_host_inflate"]
    if "gpu_bgzf" in res:
        res["gpu_bgzf_inflate_text_gbps_events"] = round(text_bytes / res["gpu_bgzf"]["inflate_ms"] / 1e6, 1)
    if "gpu_bgzf" in res and "gpu_bgzf_host_inflate" in res:
        res["speedup_bgzf_gpu_over_host_inflate"] = round(res["gpu_bgzf_host_inflate"]["total_s"] / res["gpu_bgzf"]["total_s"], 2)
        kernel_s = res["gpu_plain"]["kernel_ms"] / 1e3
        res["gpu_kernel_text_gbps_events"] = round(text_bytes / kernel_s / 1e9, 1) if kernel_s else None

    if not args.skip_cpu:
        for form, path in (("plain", plain), ("bgzf", bgz)):
            t0 = time.perf_counter()
            want = vcfio.read_vcf(path)
            res[f"cpu_{form}_s"] = round(time.perf_counter() - t0, 3)
            res[f"equal_{form}"] = same(gpu[form], want)
            res[f"speedup_{form}"] = round(res[f"cpu_{form}_s"] / res["gpu_" + (form if f"gpu_{form}" in res else "bgzf_host_inflate")]["total_s"], 2)
            del want

    if not args.skip_write:
        write_phase(args, bgz, res)

    # streaming-read calibration of this GPU (the shape the selection kernels are held against)
    with device.DeviceMatrix(2504, device=args.device) as m:
        c = m.add_chunk(2_000_000)
        m.synth_fill(c, seed=1)
        res["stream_gbps"] = round(m.stream_calibration(20), 1)
    if res.get("gpu_kernel_text_gbps_events"):
        res["kernel_text_frac_of_stream"] = round(res["gpu_kernel_text_gbps_events"] / res["stream_gbps"], 3)
    line = json.dumps(res)
    print(line)
    with open(os.path.join(args.out, "vcf_bench.json"), "w") as fh:
        fh.write(line + "\n")
    if not args.skip_cpu and not (res["equal_plain"] and res["equal_bgzf"]):
        sys.exit(1)


if __name__ == "__main__":
    main()
