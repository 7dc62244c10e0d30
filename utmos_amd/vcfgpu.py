"""VCF genotype reader on the GPU: the same dict as vcfio.read_vcf, parsed by the HIP kernels of csrc/vcf.hip.h.

The host reads the header (``##`` lines, the sample names of ``#CHROM``), then streams the records in batches cut at
the last newline: plain text straight into the parse context's pinned staging, any gzip that is not BGZF as one
stream.  BGZF (the block gzip of bgzip / htslib: gzip members with a ``BC`` extra field holding their size) is inflated
on the GPU by default (``inflate="auto"`` or ``"gpu"``, csrc/inflate.hip.h): the host inflates only the members that
hold the header, then reads compressed members straight into the staging, cut into batches at member borders, and the
device inflates, checks and parses them; a record that crosses a batch border stays on the device.  ``inflate="host"``
inflates BGZF members on a thread pool instead and cuts batches at newlines on the host.  While the GPU parses one
batch the host fills the other slot.  The kernels return per record the packed
presence row, AF, het / hom-alt counts and the singleton flag of the reference's convert (utmos/convert.py:43-88).

A ``.bcf`` path takes the BCF route (csrc/bcf.hip.h): the host reads the header -- inflating BGZF members
until the magic, ``l_text`` and the header text are complete -- and resolves GT's dictionary index (bcfio.py); the rest
of the stream goes to the device as whole BGZF members, or as stream bytes when the file is the bare stream or
``inflate="host"``.  BCF has no newline, so the device also finds the records (by their length prefixes) and keeps the
unfinished one between batches.  The result equals bcfio.read_bcf's.

Contract: for every input on which vcfio.read_vcf succeeds and whose allele tokens are all ``.`` or unsigned decimals
(below 10^18), GT, AF and samples are identical to read_vcf's.  A ``#CHROM`` line after the first record raises
ValueError (read_vcf would restart its sample list), as does every input read_vcf rejects.
"""
import ctypes
import gzip
import mmap
import os
import re
import time
import zlib
from collections import deque
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import _native as nat

DEFAULT_BATCH_BYTES = 64 << 20
INFLATE_MODES = ("auto", "gpu", "host")
BGZF_FIRST, BGZF_LAST = 1, 2          # utm_vcf_parse_bgzf flags (UTM_BGZF_FIRST, UTM_BGZF_LAST)
FLAG_SINGLETON, FLAG_SKIPPED = 1, 2   # utm_vcf_fetch flags (UTM_VCF_SINGLETON, UTM_VCF_SKIPPED)
UTM_EINVAL = -1


def inflate_threads():
    """Threads that inflate BGZF members: the CPUs this process may run on, at most 16."""
    return min(16, len(os.sched_getaffinity(0)))


# ---------------------------------------------------------------------------------------------- BGZF
def is_bgzf(head):
    """head = the first bytes of a file: a gzip member whose FEXTRA field opens with the BGZF `BC` subfield."""
    return (len(head) >= 18 and head[0] == 0x1F and head[1] == 0x8B and head[2] == 8 and head[3] & 4
            and head[12] == 0x42 and head[13] == 0x43)


def bgzf_members(buf):
    """[(offset, size, isize)] of every BGZF member of buf (size from BSIZE, isize from the member's trailer)."""
    out, off, n = [], 0, len(buf)
    while off < n:
        if n - off < 18 or buf[off] != 0x1F or buf[off + 1] != 0x8B or buf[off + 2] != 8 or not buf[off + 3] & 4:
            raise ValueError(f"not a BGZF member at byte {off}")
        xlen = int.from_bytes(buf[off + 10:off + 12], "little")
        p, end, bsize = off + 12, off + 12 + xlen, None
        while p + 4 <= end:
            slen = int.from_bytes(buf[p + 2:p + 4], "little")
            if buf[p] == 0x42 and buf[p + 1] == 0x43 and slen == 2:
                bsize = int.from_bytes(buf[p + 4:p + 6], "little")
            p += 4 + slen
        if bsize is None or off + bsize + 1 > n:
            raise ValueError(f"BGZF member at byte {off}: no BC field or truncated")
        size = bsize + 1
        out.append((off, size, int.from_bytes(buf[off + size - 4:off + size], "little")))
        off += size
    return out


class _MemberSource:
    """BGZF members inflated on the host one per fill (the header's members on the GPU path)."""

    def __init__(self, path, mm, members):
        self.path, self.mm, self.members = path, mm, members
        self.next = 0
        self.rest = b""

    def fill(self, view):
        if not self.rest:
            if self.next == len(self.members):
                return 0
            off, size, isize = self.members[self.next]
            try:
                self.rest = zlib.decompress(memoryview(self.mm)[off:off + size], 31)
            except zlib.error as err:
                raise ValueError(f"{self.path}: BGZF member at byte {off}: {err}") from None
            if len(self.rest) != isize:
                raise ValueError(f"{self.path}: BGZF member at byte {off}: {len(self.rest)} bytes inflated, ISIZE says {isize}")
            self.next += 1
        k = min(len(view), len(self.rest))
        view[:k] = self.rest[:k]
        self.rest = self.rest[k:]
        return k

    def close(self):
        pass


class _StreamSource:
    """Plain text (read straight into the staging) or a gzip stream (one inflater)."""

    def __init__(self, fh):
        self.fh = fh

    def fill(self, view):
        return self.fh.readinto(view) or 0

    def close(self):
        self.fh.close()


class _BgzfSource:
    """BGZF members inflated in parallel, each written to its place in the caller's buffer."""

    def __init__(self, path, threads, first=0):
        """first: the member to start at (those in front of it are the caller's, e.g. a header it has read)."""
        self.path = path
        self.fh = open(path, "rb")
        self.mm = mmap.mmap(self.fh.fileno(), 0, access=mmap.ACCESS_READ)
        try:
            self.members = bgzf_members(self.mm)
        except ValueError as err:
            self.mm.close()
            self.fh.close()
            raise ValueError(f"{path}: {err}") from None
        self.next = first
        self.rest = b""  # inflated bytes that did not fit the last buffer
        self.pool = ThreadPoolExecutor(max_workers=threads or inflate_threads())

    def _inflate(self, k):
        off, size, isize = self.members[k]
        try:
            data = zlib.decompress(memoryview(self.mm)[off:off + size], 31)
        except zlib.error as err:
            raise ValueError(f"{self.path}: BGZF member at byte {off}: {err}") from None
        if len(data) != isize:
            raise ValueError(f"{self.path}: BGZF member at byte {off}: {len(data)} bytes inflated, ISIZE says {isize}")
        return data

    def fill(self, view):
        room, out = len(view), 0
        if self.rest:
            k = min(room, len(self.rest))
            view[:k] = self.rest[:k]
            self.rest, out = self.rest[k:], k
        if out == room or self.next == len(self.members):
            return out
        first, at, places = self.next, out, []
        while self.next < len(self.members) and at + self.members[self.next][2] <= room:
            places.append(at)
            at += self.members[self.next][2]
            self.next += 1
        if not places:  # the next member alone is larger than the room left: keep its tail for the next call
            data = self._inflate(self.next)
            self.next += 1
            k = room - out
            view[out:room] = data[:k]
            self.rest = data[k:]
            return room
        arr = np.frombuffer(view, dtype=np.uint8)

        def put(i):
            data = self._inflate(first + i)
            arr[places[i]:places[i] + len(data)] = np.frombuffer(data, dtype=np.uint8)

        for _ in self.pool.map(put, range(len(places))):
            pass
        return at

    def close(self):
        self.pool.shutdown()
        self.mm.close()
        self.fh.close()


def open_source(path, threads=None):
    """A .fill(view) -> bytes-written reader of the file's text (read_vcf's rule: gzip when the name ends in .gz)."""
    if path.endswith(".gz"):
        with open(path, "rb") as fh:
            head = fh.read(18)
        if is_bgzf(head):
            return _BgzfSource(path, threads)
        return _StreamSource(gzip.open(path, "rb"))
    return _StreamSource(open(path, "rb", buffering=0))


def _last_newline(arr, n):
    """Offset of the last '\\n' in arr[:n], or -1."""
    hi = n
    while hi > 0:
        lo = max(0, hi - (1 << 16))
        hit = np.flatnonzero(arr[lo:hi] == 10)
        if len(hit):
            return lo + int(hit[-1])
        hi = lo
    return -1


# ---------------------------------------------------------------------------------------------- reader
class GpuVcfReader:
    """A parse context on one GPU, reusable across files (it is rebuilt only when the sample count changes)."""

    def __init__(self, device=0, batch_bytes=DEFAULT_BATCH_BYTES, threads=None, inflate="auto"):
        """inflate: where BGZF members are inflated -- "auto" / "gpu" on the device, "host" on a thread pool.  "gpu"
        on a gzip file that is not BGZF raises ValueError; plain text and single-stream gzip read the same either way."""
        if inflate not in INFLATE_MODES:
            raise ValueError(f"inflate={inflate!r}: one of {', '.join(INFLATE_MODES)}")
        self.device, self.batch_bytes, self.threads, self.inflate = int(device), int(batch_bytes), threads, inflate
        self.handle, self.n_samples = None, None
        self.timing = {}
        self.kernel_timing = {}

    def close(self):
        if self.handle is not None:
            nat.lib().utm_vcf_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _context(self, n_samples):
        if self.handle is not None and self.n_samples == n_samples:
            return self.handle
        self.close()
        h = ctypes.c_void_p()
        nat.check(nat.lib().utm_vcf_create(self.device, n_samples, self.batch_bytes, ctypes.byref(h)))
        self.handle, self.n_samples = h, n_samples
        return h

    @staticmethod
    def _header(path, src):
        """-> (samples, header lines, the bytes after the #CHROM line)."""
        buf, n_lines, pos, eof = bytearray(), 0, 0, False
        chunk = bytearray(1 << 20)
        while True:
            nl = buf.find(b"\n", pos)
            if nl < 0:
                if eof:
                    if pos == len(buf):
                        raise ValueError(f"{path}: no #CHROM header line")
                    buf += b"\n"
                    continue
                k = src.fill(memoryview(chunk))
                if k == 0:
                    eof = True
                buf += chunk[:k]
                continue
            raw = bytes(buf[pos:nl + 1])
            pos, n_lines = nl + 1, n_lines + 1
            if raw.startswith(b"##"):
                continue
            raw = raw.rstrip(b"\r\n")
            if raw.startswith(b"#CHROM"):
                return np.array(raw.decode().split("\t")[9:], dtype=str), n_lines, bytes(buf[pos:])
            if raw:
                raise ValueError(f"{path}: a record in front of the #CHROM header line")

    def read(self, path):
        """-> {'GT', 'AF' (n, 1), 'samples', 'stats': {'num_het', 'num_hom'}, 'singleton' (n,) bool}; self.timing holds
        the phase split of this call (seconds: fill = read / inflate on the host -- with BGZF inflated on the GPU, reading
        the compressed bytes; ms: h2d, kernels, d2h, inflate = the GPU inflate kernels).  self.kernel_timing splits kernel_ms into find_ms
        (finding the records: newline count and scan, or k_bcf_chain) and parse_ms (parsing them)."""
        lib = nat.lib()
        t0 = time.perf_counter()
        if path.endswith(".bcf"):
            return self._read_bcf(path, t0)
        if path.endswith(".gz") and self.inflate != "host":
            with open(path, "rb") as fh:
                bgzf = is_bgzf(fh.read(18))
            if bgzf:
                return self._read_bgzf(path, t0)
            if self.inflate == "gpu":
                raise ValueError(f"{path}: inflate='gpu' needs BGZF (bgzip) input; this gzip file is one stream")
        src = open_source(path, self.threads)
        fill_s = 0.0
        try:
            samples, n_head, carry = self._header(path, src)
            if len(samples) == 0:
                return self._no_samples(path, src, samples, carry)
            h = self._context(len(samples))
            width = (len(samples) + 7) // 8

            def batches(carry):
                eof = False
                while True:
                    ptr, cap = ctypes.c_void_p(), ctypes.c_uint64()
                    nat.check(lib.utm_vcf_staging(h, max(self.batch_bytes, len(carry) + 1), ctypes.byref(ptr), ctypes.byref(cap)))
                    arr = np.ctypeslib.as_array((ctypes.c_uint8 * cap.value).from_address(ptr.value))
                    arr[:len(carry)] = np.frombuffer(carry, dtype=np.uint8)
                    n = len(carry)
                    tf = time.perf_counter()
                    while True:
                        while n < len(arr) - 1 and not eof:   # (one byte kept for a final newline)
                            k = src.fill(memoryview(arr)[n:len(arr) - 1])
                            eof, n = k == 0, n + k
                        cut = _last_newline(arr, n)
                        if eof and cut != n - 1 and n:        # the last record has no newline
                            arr[n] = 10
                            n += 1
                            cut = n - 1
                        if cut >= 0 or eof:
                            break
                        # one record longer than the batch: grow the staging (it keeps its contents) and read on
                        nat.check(lib.utm_vcf_staging(h, 2 * len(arr), ctypes.byref(ptr), ctypes.byref(cap)))
                        arr = np.ctypeslib.as_array((ctypes.c_uint8 * cap.value).from_address(ptr.value))
                    fill = time.perf_counter() - tf
                    if cut < 0:
                        return
                    carry = arr[cut + 1:n].tobytes()
                    n_rec = ctypes.c_uint64()
                    nat.check(lib.utm_vcf_parse(h, ptr, cut + 1, ctypes.byref(n_rec)))
                    yield n_rec.value, fill
                    if eof and not carry:
                        return

            parts = self._pipeline(path, h, width, n_head, batches(carry), t0)
        finally:
            src.close()
        return self._assemble(parts, samples, width)

    def _read_bgzf(self, path, t0):
        """BGZF inflated on the GPU: members after the header's go to the device compressed, in batches of whole
        members (ISIZE summed up to batch_bytes); the device keeps a record that crosses a batch border."""
        lib = nat.lib()
        with open(path, "rb") as fh, mmap.mmap(fh.fileno(), 0, access=mmap.ACCESS_READ) as mm:
            try:
                members = bgzf_members(mm)
            except ValueError as err:
                raise ValueError(f"{path}: {err}") from None
            hs = _MemberSource(path, mm, members)
            samples, n_head, prefix = self._header(path, hs)
            prefix += hs.rest
            if len(samples) == 0:
                return self._no_samples(path, hs, samples, prefix)
            h = self._context(len(samples))
            width = (len(samples) + 7) // 8
            batches = self._member_batches(path, fh, h, members, hs.next, prefix, lib.utm_vcf_parse_bgzf)
            parts = self._pipeline(path, h, width, n_head, batches, t0)
        return self._assemble(parts, samples, width)

    def _member_batches(self, path, fh, h, members, j, prefix, parse, *key):
        """Whole BGZF members from member j on, read compressed into the staging in batches (ISIZE summed up to
        batch_bytes, at least one member) and queued with `parse` (utm_vcf_parse_bgzf, or utm_vcf_parse_bcf with its
        key); `prefix` = text the host already holds, in front of the first batch."""
        lib = nat.lib()
        table = np.array(members, dtype=np.int64).reshape(-1, 3)
        off, size, isize = table[:, 0], table[:, 1], table[:, 2]
        ends = np.cumsum(isize)
        pre = np.frombuffer(prefix, dtype=np.uint8) if prefix else None
        flags, done = BGZF_FIRST, 0
        while True:
            k = j
            if j < len(members):   # whole members, their text summed up to batch_bytes (at least one)
                base = ends[j - 1] if j else 0
                k = max(j + 1, int(np.searchsorted(ends, base + self.batch_bytes, side="right")))
            last = k == len(members)
            packed = int(off[k - 1] + size[k - 1] - off[j]) if k > j else 0
            tf = time.perf_counter()
            ptr, cap = ctypes.c_void_p(), ctypes.c_uint64()
            nat.check(lib.utm_vcf_staging(h, max(packed, 1), ctypes.byref(ptr), ctypes.byref(cap)))
            if packed:
                view = memoryview((ctypes.c_uint8 * packed).from_address(ptr.value)).cast("B")
                fh.seek(int(off[j]))
                got = 0
                while got < packed:
                    n = fh.readinto(view[got:])
                    if not n:
                        raise ValueError(f"{path}: truncated")
                    got += n
            mem = np.ascontiguousarray(np.stack([size[j:k], isize[j:k]], axis=1), dtype=np.uint32)
            fill = time.perf_counter() - tf
            n_rec, carry = ctypes.c_uint64(), ctypes.c_uint64()
            rc = parse(h, pre.ctypes.data if pre is not None else None, len(pre) if pre is not None else 0, ptr, packed,
                       mem.ctypes.data, k - j, *key, flags | (BGZF_LAST if last else 0), ctypes.byref(n_rec),
                       ctypes.byref(carry))
            if rc == UTM_EINVAL:
                raise ValueError(f"{path}: {self._batch_error(done, lambda i: int(off[j + i]))}")
            nat.check(rc)
            yield n_rec.value, fill
            flags, pre, j, done = 0, None, k, done + n_rec.value
            if last:
                return

    @staticmethod
    def _batch_error(done, member_at=None):
        """utm_last_error() of a failed parse call, with the member's place in the file and the record's number in it
        (`done` = records of the batches before)."""
        msg = nat.lib().utm_last_error().decode("utf-8", "replace")
        m = re.match(r"member (\d+) of the batch: (.*)", msg)
        if m and member_at:
            return f"BGZF member at byte {member_at(int(m.group(1)))}: {m.group(2)}"
        m = re.match(r"record (\d+) of the batch: (.*)", msg)
        if m:
            return f"record {done + int(m.group(1)) + 1}: {m.group(2)}"
        m = re.match(r"truncated record: the stream ends (\d+) bytes into record (\d+) of the batch", msg)
        if m:
            return f"record {done + int(m.group(2)) + 1}: truncated record (the file ends {m.group(1)} bytes into it)"
        return msg

    def _read_bcf(self, path, t0):
        """A .bcf file: BGZF (members inflated on the GPU, or on the thread pool with inflate="host") or the bare
        stream.  The host reads the header; the device finds and parses the records."""
        from . import bcfio
        lib = nat.lib()
        if os.path.getsize(path) == 0:
            raise ValueError(f"{path}: an empty file")
        with open(path, "rb") as fh, mmap.mmap(fh.fileno(), 0, access=mmap.ACCESS_READ) as mm:
            head = bytes(mm[:18])
            raw = head[:3] == bcfio.MAGIC[:3]
            if not raw and not is_bgzf(head):
                raise ValueError(f"{path}: neither a BCF stream (magic BCF\\x02) nor a BGZF container")
            if raw:
                members, src = None, _StreamSource(open(path, "rb", buffering=0))
            else:
                try:
                    members = bgzf_members(mm)
                except ValueError as err:
                    raise ValueError(f"{path}: {err}") from None
                src = _MemberSource(path, mm, members)
            try:
                samples, ids, prefix = bcfio.read_header(path, src.fill)
                if len(samples) == 0:
                    return self._no_samples_bcf(path, t0)
                gt_key = ids.get("GT", bcfio.NO_KEY)
                h = self._context(len(samples))
                width = (len(samples) + 7) // 8
                if members is not None and self.inflate != "host":
                    batches = self._member_batches(path, fh, h, members, src.next, prefix + src.rest,
                                                   lib.utm_vcf_parse_bcf, gt_key)
                    parts = self._pipeline(path, h, width, None, batches, t0)
                else:
                    if members is not None:    # the members after the header's, inflated on the thread pool
                        prefix, src = prefix + src.rest, _BgzfSource(path, self.threads, first=src.next)
                    parts = self._pipeline(path, h, width, None, self._stream_batches(path, h, src, prefix, gt_key), t0)
            finally:
                src.close()
        return self._assemble(parts, samples, width)

    def _no_samples_bcf(self, path, t0):
        """The header names no sample: there is no GT matrix and no parse context for it (utm_vcf_create wants a
        sample).  The records are still checked -- each must say n_sample = 0 -- by bcfio on the host, which is the one
        place a .bcf is not read on the GPU; self.timing says so with zero device times."""
        from . import bcfio
        t1 = time.perf_counter()
        out = bcfio.read_bcf(path)
        self.timing = {"fill_s": time.perf_counter() - t1, "h2d_ms": 0.0, "kernel_ms": 0.0,
                       "d2h_ms": 0.0, "inflate_ms": 0.0, "total_s": time.perf_counter() - t0}
        self.kernel_timing = {"find_ms": 0.0, "parse_ms": 0.0}
        return out

    def _stream_batches(self, path, h, src, prefix, gt_key):
        """Stream bytes the host holds (the bare stream, or members it inflated), batch_bytes per batch."""
        lib = nat.lib()
        pre = np.frombuffer(prefix, dtype=np.uint8) if prefix else None
        flags, done, eof = BGZF_FIRST, 0, False
        while True:
            tf = time.perf_counter()
            ptr, cap = ctypes.c_void_p(), ctypes.c_uint64()
            nat.check(lib.utm_vcf_staging(h, self.batch_bytes, ctypes.byref(ptr), ctypes.byref(cap)))
            view = memoryview((ctypes.c_uint8 * self.batch_bytes).from_address(ptr.value)).cast("B")
            n = 0
            while n < self.batch_bytes and not eof:
                k = src.fill(view[n:])
                eof, n = k == 0, n + k
            fill = time.perf_counter() - tf
            n_rec, carry = ctypes.c_uint64(), ctypes.c_uint64()
            rc = lib.utm_vcf_parse_bcf(h, pre.ctypes.data if pre is not None else None, len(pre) if pre is not None else 0,
                                       ptr, n, None, 0, gt_key, flags | (BGZF_LAST if eof else 0), ctypes.byref(n_rec),
                                       ctypes.byref(carry))
            if rc == UTM_EINVAL:
                raise ValueError(f"{path}: {self._batch_error(done)}")
            nat.check(rc)
            yield n_rec.value, fill
            flags, pre, done = 0, None, done + n_rec.value
            if eof:
                return

    def _pipeline(self, path, h, width, n_head, batches, t0):
        """Runs the batches through the context's two slots -> the fetched parts, and sets self.timing.  n_head = the
        header's lines (errors name a line), or None for BCF (errors name a record, counted from the first).  `batches`
        stages and queues one batch per step and yields (its records, seconds spent filling its staging); it is
        resumed only once a slot is free for the next batch."""
        lib = nat.lib()
        ms0, inf0, k0 = (ctypes.c_double * 3)(), ctypes.c_double(), (ctypes.c_double * 2)()
        nat.check(lib.utm_vcf_timing(h, ms0))
        nat.check(lib.utm_vcf_kernel_timing(h, k0))
        nat.check(lib.utm_vcf_inflate_timing(h, ctypes.byref(inf0)))
        pending, parts, line_base, fill_s = deque(), [], 0, 0.0
        try:
            it = iter(batches)
            while True:
                try:
                    n_rec, fill = next(it)
                except StopIteration:
                    break
                except ValueError:
                    # a parse call failed: a batch queued before it may hold an earlier bad record, whose error comes first
                    while pending:
                        self._fetch(path, h, width, n_head, *pending.popleft())
                    raise
                pending.append((n_rec, line_base))
                line_base += n_rec
                fill_s += fill
                if len(pending) == 2:
                    parts.append(self._fetch(path, h, width, n_head, *pending.popleft()))
            while pending:
                parts.append(self._fetch(path, h, width, n_head, *pending.popleft()))
        finally:
            while pending:                 # drain the other slot: the context stays usable after a failure
                pending.popleft()
                lib.utm_vcf_fetch(h, None, None, None, None, None)
        ms1, inf1, k1 = (ctypes.c_double * 3)(), ctypes.c_double(), (ctypes.c_double * 2)()
        nat.check(lib.utm_vcf_timing(h, ms1))
        nat.check(lib.utm_vcf_kernel_timing(h, k1))
        nat.check(lib.utm_vcf_inflate_timing(h, ctypes.byref(inf1)))
        self.kernel_timing = {"find_ms": k1[0] - k0[0], "parse_ms": k1[1] - k0[1]}
        self.timing = {"fill_s": fill_s, "h2d_ms": ms1[0] - ms0[0], "kernel_ms": ms1[1] - ms0[1],
                       "d2h_ms": ms1[2] - ms0[2], "inflate_ms": inf1.value - inf0.value,
                       "total_s": time.perf_counter() - t0}
        return parts

    def _fetch(self, path, h, width, n_head, n_rec, line_base):
        rows = np.empty((n_rec, width), dtype=np.uint8)
        af = np.empty(n_rec, dtype=np.float64)
        het = np.empty(n_rec, dtype=np.uint32)
        hom = np.empty(n_rec, dtype=np.uint32)
        flags = np.empty(n_rec, dtype=np.uint8)
        rc = nat.lib().utm_vcf_fetch(h, rows.ctypes.data, af.ctypes.data, het.ctypes.data, hom.ctypes.data,
                                     flags.ctypes.data)
        if rc == UTM_EINVAL:                             # a malformed record
            msg = nat.lib().utm_last_error().decode("utf-8", "replace")
            m = re.match(r"record (\d+) of the batch: (.*)", msg)
            if m:
                at = line_base + int(m.group(1)) + 1
                msg = f"record {at}: {m.group(2)}" if n_head is None else f"line {n_head + at}: {m.group(2)}"
            raise ValueError(f"{path}: {msg}")
        nat.check(rc)
        keep = (flags & FLAG_SKIPPED) == 0
        return rows[keep], af[keep], het[keep], hom[keep], (flags[keep] & FLAG_SINGLETON) != 0

    @staticmethod
    def _assemble(parts, samples, width):
        if parts:
            rows, af, het, hom, sing = (np.concatenate(x) for x in zip(*parts))
        else:
            rows, af = np.zeros((0, width), np.uint8), np.zeros(0, np.float64)
            het = hom = np.zeros(0, np.uint32)
            sing = np.zeros(0, bool)
        return {"GT": rows, "AF": af.reshape(-1, 1), "samples": samples,
                "stats": {"num_het": np.int64(het.sum(dtype=np.int64)), "num_hom": np.int64(hom.sum(dtype=np.int64))},
                "het": het, "hom": hom, "singleton": sing}

    def _no_samples(self, path, src, samples, carry):
        """#CHROM names no sample: no record can be valid (read_vcf: every record fails its cell count)."""
        chunk = bytearray(1 << 20)
        text = bytearray(carry)
        while True:
            k = src.fill(memoryview(chunk))
            if not k:
                break
            text += chunk[:k]
        for raw in bytes(text).split(b"\n"):
            if not raw.startswith(b"##") and raw.rstrip(b"\r"):
                raise ValueError(f"{path}: a record, but the header names no sample")
        return self._assemble([], samples, 0)


def read_vcf(path, device=0, batch_bytes=DEFAULT_BATCH_BYTES, threads=None, inflate="auto"):
    """One file through a fresh GpuVcfReader: vcfio.read_vcf's dict plus 'stats' and 'singleton'."""
    with GpuVcfReader(device, batch_bytes, threads, inflate) as reader:
        return reader.read(path)


def bgzf_compress(data, level=6, threads=None, block=0xFF00):
    """data -> BGZF bytes (members of at most `block` input bytes, then the empty end-of-file member), compressed by a
    thread pool: what bgzip writes, for tests and the benchmark's synthetic call sets."""
    view = memoryview(data)

    def member(off):
        piece = view[off:off + block]
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        body = c.compress(piece) + c.flush()
        head = b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + (len(body) + 25).to_bytes(2, "little")
        return head + body + zlib.crc32(piece).to_bytes(4, "little") + len(piece).to_bytes(4, "little")

    with ThreadPoolExecutor(max_workers=threads or inflate_threads()) as pool:
        parts = list(pool.map(member, range(0, len(data), block)))
    return b"".join(parts) + member(len(data))
