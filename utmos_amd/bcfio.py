"""Minimal BCF2 genotype reader on the CPU: for a BCF file, the dict vcfio.read_vcf gives for the VCF text of the same
calls (plus the het / hom-alt / singleton extras of vcfgpu.read_vcf).  It is the numpy restatement the GPU reader
(vcfgpu.py, csrc/bcf.hip.h) is tested against, and holds the header and dictionary parser that reader uses.

The format subset is DESIGN §8.4: a BGZF container or the bare stream; magic ``BCF\\2`` + minor 1 or 2, ``l_text``, the
VCF header text, then records ``l_shared, l_indiv, shared block, individual block``.  Of a record only n_allele, n_fmt,
n_sample and the GT field are read.  No file written by htslib has been read with it.
"""
import gzip
import re
import struct
import zlib

import numpy as np

MAGIC = b"BCF\x02"
TYPE_SIZE = {0: 0, 1: 1, 2: 2, 3: 4, 5: 4, 7: 1}
MAX_ALT = 4096
NO_KEY = 0xFFFFFFFF   # GT's key when the header declares no GT: no field's key equals it, so every record fails

# the reasons of csrc/host_vcf.hip.h (vcf_error_text), word for word
E_SHARED = "l_shared below 24"
E_TRUNC = "truncated record"
E_NSAMPLE = "a record whose n_sample differs from the header's sample count"
E_NALT = "more alt alleles than the parser holds (4096)"
E_FIELD = "a FORMAT field that runs past l_indiv"
E_TYPE = "an unknown type code"
E_GT_TYPE = "a GT field that is not of an integer type"
E_NO_GT = "no GT among the FORMAT fields"


class RecordError(ValueError):
    """A malformed record: .index counts from the first record of the stream (0-based), .reason says what."""

    def __init__(self, index, reason):
        super().__init__(f"record {index + 1}: {reason}")
        self.index, self.reason = index, reason


# ---------------------------------------------------------------------------------------------- header
def parse_header_text(text):
    """The header text (``##`` lines and ``#CHROM``; NUL-terminated or not) -> (samples, {ID: dictionary index}).
    IDX= gives a line's index; without it PASS is 0 and every new ID takes the next index in order of first appearance,
    one numbering over ##FILTER, ##INFO and ##FORMAT."""
    ids = {"PASS": 0}
    samples = None
    for line in bytes(text).rstrip(b"\x00").decode().splitlines():
        m = re.match(r"##(FILTER|INFO|FORMAT)=<(.*)>\s*$", line)
        if m:
            fields = dict(re.findall(r"(\w+)=(\"[^\"]*\"|[^,]*)", m.group(2)))
            if "ID" not in fields:
                continue
            if "IDX" in fields:
                ids[fields["ID"]] = int(fields["IDX"])
            elif fields["ID"] not in ids:
                ids[fields["ID"]] = max(ids.values()) + 1
        elif line.startswith("#CHROM"):
            samples = np.array(line.rstrip("\r").split("\t")[9:], dtype=str)
    if samples is None:
        raise ValueError("no #CHROM line in the BCF header text")
    return samples, ids


def read_header(path, fill):
    """fill(memoryview) -> bytes written (0 at the end): the stream from its first byte.
    -> (samples, dictionary, the stream bytes read beyond the header)."""
    buf, chunk = bytearray(), bytearray(1 << 20)

    def need(n):
        while len(buf) < n:
            k = fill(memoryview(chunk))
            if not k:
                raise ValueError(f"{path}: the BCF header is truncated")
            buf.extend(chunk[:k])

    need(9)
    if bytes(buf[:4]) != MAGIC or buf[4] not in (1, 2):
        raise ValueError(f"{path}: bad magic {bytes(buf[:5])!r} (expected BCF\\x02 and minor version 1 or 2)")
    l_text = struct.unpack_from("<I", buf, 5)[0]
    need(9 + l_text)
    try:
        samples, ids = parse_header_text(buf[9:9 + l_text])
    except ValueError as err:
        raise ValueError(f"{path}: {err}") from None
    return samples, ids, bytes(buf[9 + l_text:])


# ---------------------------------------------------------------------------------------------- records
def _int_scalar(buf, p, e):
    """A typed integer scalar at p -> (value, the byte after it), or None when there is none below e."""
    if p >= e:
        return None
    d = buf[p]
    if d >> 4 != 1 or d & 15 not in (1, 2, 3):
        return None
    w = TYPE_SIZE[d & 15]
    if p + 1 + w > e:
        return None
    return int.from_bytes(buf[p + 1:p + 1 + w], "little"), p + 1 + w


def find_gt(buf, o, n_samp, gt_key):
    """The record at o (whole, l_shared >= 24) -> (n_alt, width, length, offset of the first GT value); width 0 = an
    empty GT field.  Raises ValueError(reason)."""
    l_shared, l_indiv = struct.unpack_from("<II", buf, o)
    e = o + 8 + l_shared + l_indiv
    n_allele = struct.unpack_from("<I", buf, o + 24)[0] >> 16
    fs = struct.unpack_from("<I", buf, o + 28)[0]
    if fs & 0xFFFFFF != n_samp:
        raise ValueError(E_NSAMPLE)
    n_alt = max(n_allele - 1, 1)
    if n_alt > MAX_ALT:
        raise ValueError(E_NALT)
    p = o + 8 + l_shared
    for _ in range(fs >> 24):
        got = _int_scalar(buf, p, e)
        if got is None or got[1] >= e:
            raise ValueError(E_FIELD)
        key, p = got
        d = buf[p]
        p += 1
        typ, length = d & 15, d >> 4
        if length == 15:
            got = _int_scalar(buf, p, e)
            if got is None:
                raise ValueError(E_FIELD)
            length, p = got
        if typ not in TYPE_SIZE:
            raise ValueError(E_TYPE)
        if length > 0x7FFFFFFF:
            raise ValueError(E_FIELD)
        size = n_samp * length * TYPE_SIZE[typ]
        if size > e - p:
            raise ValueError(E_FIELD)
        if key == gt_key:
            if typ in (5, 7):
                raise ValueError(E_GT_TYPE)
            return n_alt, (TYPE_SIZE[typ] if length else 0), length, p
        p += size
    raise ValueError(E_NO_GT)


def decode_gt(buf, n_samp, n_alt, width, length, at):
    """-> (presence (S,) bool, allele counts (n_alt + 1,), het cells, hom-alt cells)."""
    counts = np.zeros(n_alt + 1, dtype=np.int64)
    if width == 0 or n_samp == 0:
        return np.zeros(n_samp, dtype=bool), counts, 0, 0
    v = np.frombuffer(buf, dtype={1: "<u1", 2: "<u2", 4: "<u4"}[width], count=n_samp * length, offset=at)
    v = v.reshape(n_samp, length).astype(np.int64)
    miss_s = 1 << (8 * width - 1)
    valid = np.logical_not(np.maximum.accumulate(v == miss_s + 1, axis=1))   # in front of the first end-of-vector
    miss = (v == miss_s) | ((v >> 1) == 0)
    a = (v >> 1) - 1
    counts += np.bincount(a[valid & ~miss & (a <= n_alt)], minlength=n_alt + 1)
    ploidy = valid.sum(axis=1)
    called = (ploidy >= 2) & ~(valid & miss).any(axis=1)
    first = a[:, 0]
    diff = (valid & (a != first[:, None])).any(axis=1)
    het = called & diff
    hom = called & ~diff & (first > 0)
    return het | hom, counts, int(het.sum()), int(hom.sum())


def parse_stream(buf, n_samp, gt_key):
    """buf = the stream bytes after the header -> (rows, af, het, hom, singleton).  Raises RecordError."""
    rows, afs, hets, homs, sing = [], [], [], [], []
    o, n = 0, len(buf)
    while o < n:
        i = len(rows)
        if n - o < 8:
            raise RecordError(i, E_TRUNC)
        l_shared, l_indiv = struct.unpack_from("<II", buf, o)
        if l_shared < 24:
            raise RecordError(i, E_SHARED)
        if o + 8 + l_shared + l_indiv > n:
            raise RecordError(i, E_TRUNC)
        try:
            n_alt, width, length, at = find_gt(buf, o, n_samp, gt_key)
        except RecordError:
            raise
        except ValueError as err:
            raise RecordError(i, str(err)) from None
        pres, counts, het, hom = decode_gt(buf, n_samp, n_alt, width, length, at)
        total = counts.sum()
        afs.append((counts[1:] / total).max() if total else 0.0)
        rows.append(np.packbits(pres))
        hets.append(het)
        homs.append(hom)
        sing.append(bool(counts[1] == 1 or counts[0] == 1))
        o += 8 + l_shared + l_indiv
    width = (n_samp + 7) // 8
    return (np.array(rows, dtype=np.uint8).reshape(len(rows), width), np.array(afs, dtype=np.float64),
            np.array(hets, dtype=np.uint32), np.array(homs, dtype=np.uint32), np.array(sing, dtype=bool))


def stream_of(path):
    """The file's BCF stream: the file itself when it opens with the magic, else the text of its BGZF members."""
    with open(path, "rb") as fh:
        data = fh.read()
    if data[:3] == MAGIC[:3]:
        return data
    if len(data) >= 18 and data[:4] == b"\x1f\x8b\x08\x04" and data[12:14] == b"BC":
        try:
            return gzip.decompress(data)
        except (OSError, EOFError, zlib.error) as err:
            raise ValueError(f"{path}: {err}") from None
    raise ValueError(f"{path}: neither a BCF stream (magic BCF\\x02) nor a BGZF container")


def read_bcf(path):
    """-> {'GT', 'AF' (n, 1), 'samples', 'stats': {'num_het', 'num_hom'}, 'het', 'hom', 'singleton'}: GT, AF and samples
    as vcfio.read_vcf gives them for the VCF text of the same calls, the rest as vcfgpu.read_vcf."""
    data = stream_of(path)
    pos = [0]

    def fill(view):
        k = min(len(view), len(data) - pos[0])
        view[:k] = data[pos[0]:pos[0] + k]
        pos[0] += k
        return k

    samples, ids, rest = read_header(path, fill)
    body = rest + data[pos[0]:]
    try:
        rows, af, het, hom, sing = parse_stream(body, len(samples), ids.get("GT", NO_KEY))
    except RecordError as err:
        raise ValueError(f"{path}: {err}") from None
    return {"GT": rows, "AF": af.reshape(-1, 1), "samples": samples,
            "stats": {"num_het": np.int64(het.sum(dtype=np.int64)), "num_hom": np.int64(hom.sum(dtype=np.int64))},
            "het": het, "hom": hom, "singleton": sing}


def parse_host(body, n_samp, gt_key):
    """parse_stream through the CPU build of the device code (utm_bcf_parse_host); the whole of `body` must be records."""
    import ctypes

    from . import _native as nat
    lib = nat.lib()
    buf = np.frombuffer(bytes(body), dtype=np.uint8)
    n_rec, carry = ctypes.c_uint64(), ctypes.c_uint64()
    nat.check(lib.utm_bcf_parse_host(buf.ctypes.data, len(buf), n_samp, gt_key, 0, None, None, None, None, None,
                                     ctypes.byref(n_rec), ctypes.byref(carry)))
    n = n_rec.value
    if carry.value:
        raise RecordError(n, E_TRUNC)
    width = (n_samp + 7) // 8
    rows = np.zeros((n, width), dtype=np.uint8)
    af, het, hom = np.zeros(n, np.float64), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    flags = np.zeros(n, np.uint8)
    rc = lib.utm_bcf_parse_host(buf.ctypes.data, len(buf), n_samp, gt_key, n, rows.ctypes.data, af.ctypes.data,
                                het.ctypes.data, hom.ctypes.data, flags.ctypes.data, ctypes.byref(n_rec),
                                ctypes.byref(carry))
    if rc == -1:
        msg = lib.utm_last_error().decode("utf-8", "replace")
        m = re.match(r"record (\d+) of the batch: (.*)", msg)
        if m:
            raise RecordError(int(m.group(1)), m.group(2))
        raise ValueError(msg)
    nat.check(rc)
    return rows, af, het, hom, (flags & 1) != 0
