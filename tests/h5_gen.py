"""Test helper: writes the subset of HDF5 that the reference's `--lowmem` store uses (utmos_amd/h5store.py reads it):
superblock 0, a symbol-table root group, v1 object headers, and datasets `data`, `samples`, `var_count` chunked
(layout v3, v1 chunk B-tree) with LZF (filter 32000) or no filter.  It covers what the two reference fixtures do not:
raw chunks (filter mask bit 0), B-trees of more than one level (more than 64 chunks), absent chunks, partial last
chunks, one-row chunks, all-zero float rows and rows with mixed values.  Includes a small LZF compressor."""
import struct

import numpy as np

UNDEF = 0xFFFFFFFFFFFFFFFF
BTREE_FANOUT = 64      # 2 x the default indexed-storage K (32)


def lzf_compress(data):
    """Greedy liblzf-format compressor (3-byte hash of the last position, matches of 3..264 bytes, 8 KiB back)."""
    data = bytes(data)
    n = len(data)
    out, lit, table = bytearray(), bytearray(), {}
    i = 0

    def flush():
        while lit:
            take = lit[:32]
            out.append(len(take) - 1)
            out.extend(take)
            del lit[:32]

    while i < n:
        ref = None
        if i + 2 < n:
            key = data[i:i + 3]
            ref = table.get(key)
            table[key] = i
        if ref is not None and i - ref <= 8192:
            top = min(264, n - i)
            length = 3
            while length < top:
                step = min(32, top - length)
                if data[ref + length:ref + length + step] == data[i + length:i + length + step]:
                    length += step
                    continue
                while length < top and data[ref + length] == data[i + length]:
                    length += 1
                break
            flush()
            off = i - ref - 1
            if length - 2 < 7:
                out.append((length - 2) << 5 | off >> 8)
            else:
                out.append(7 << 5 | off >> 8)
                out.append(length - 9)
            out.append(off & 255)
            i += length
        else:
            lit.append(data[i])
            i += 1
    flush()
    return bytes(out)


class _File:
    def __init__(self):
        self.buf = bytearray(96)                         # the superblock is written last

    def put(self, blob, align=8):
        while len(self.buf) % align:
            self.buf.append(0)
        at = len(self.buf)
        self.buf.extend(blob)
        return at


def _msg(mtype, body, flags=0):
    body = bytes(body)
    body += b"\0" * (-len(body) % 8)
    return struct.pack("<HHB3x", mtype, len(body), flags) + body


def _object_header(f, messages, split=False):
    """v1 object header; split=True puts every message after the first into a continuation block."""
    msgs = [_msg(t, b) for t, b in messages]
    if split and len(msgs) > 1:
        rest = b"".join(msgs[1:])
        cont_at = f.put(rest)
        first = msgs[0] + _msg(0x10, struct.pack("<QQ", cont_at, len(rest)))
        return f.put(struct.pack("<BBHII4x", 1, 0, len(msgs) + 1, 1, len(first)) + first)
    body = b"".join(msgs)
    return f.put(struct.pack("<BBHII4x", 1, 0, len(msgs), 1, len(body)) + body)


def _dataspace(shape, maxshape):
    body = struct.pack("<BBB5x", 1, len(shape), 1)
    body += b"".join(struct.pack("<Q", d) for d in shape)
    body += b"".join(struct.pack("<Q", UNDEF if d is None else d) for d in maxshape)
    return body


def _datatype(kind, size):
    if kind == "bool":                                     # h5py's bool: enum FALSE = 0, TRUE = 1 over int8
        base = bytes([0x10, 0x08, 0, 0]) + struct.pack("<IHH", 1, 0, 8)
        names = b"".join(n + b"\0" * (8 - len(n)) for n in (b"FALSE", b"TRUE"))
        return bytes([0x18, 2, 0, 0]) + struct.pack("<I", 1) + base + names + bytes([0, 1])
    if kind == "float":
        if size == 8:
            return bytes([0x11, 0x20, 0x3F, 0]) + struct.pack("<IHHBBBBI", 8, 0, 64, 52, 11, 0, 52, 1023)
        return bytes([0x11, 0x20, 0x1F, 0]) + struct.pack("<IHHBBBBI", 4, 0, 32, 23, 8, 0, 23, 127)
    if kind == "int":
        return bytes([0x10, 0x08, 0, 0]) + struct.pack("<IHH", size, 0, size * 8)
    if kind == "string":
        return bytes([0x13, 0x01, 0, 0]) + struct.pack("<I", size)
    raise ValueError(kind)


def _chunk_btree(f, entries, rank):
    """entries: [(row, stored size, mask, address)] sorted by row -> root address of a v1 type-1 B-tree."""
    def key(size, mask, row):
        return struct.pack("<II", size, mask) + struct.pack(f"<{rank + 1}Q", row, *([0] * rank))

    level, nodes = 0, []
    for k in range(0, len(entries), BTREE_FANOUT):         # leaves: (first key, last key, address)
        part = entries[k:k + BTREE_FANOUT]
        body = b"".join(key(s, m, r) + struct.pack("<Q", a) for r, s, m, a in part) + key(0, 0, part[-1][0] + 1)
        at = f.put(b"TREE" + struct.pack("<BBHQQ", 1, level, len(part), UNDEF, UNDEF) + body)
        nodes.append((key(part[0][1], part[0][2], part[0][0]), key(0, 0, part[-1][0] + 1), at))
    while len(nodes) > 1:
        level += 1
        upper = []
        for k in range(0, len(nodes), BTREE_FANOUT):
            part = nodes[k:k + BTREE_FANOUT]
            body = b"".join(first + struct.pack("<Q", a) for first, _last, a in part) + part[-1][1]
            at = f.put(b"TREE" + struct.pack("<BBHQQ", 1, level, len(part), UNDEF, UNDEF) + body)
            upper.append((part[0][0], part[-1][1], at))
        nodes = upper
    return nodes[0][2]


def _dataset(f, kind, size, shape, maxshape, chunk_shape, chunks, filtered=True, split=False):
    """chunks: [(first row, stored blob, mask)] -> object header address."""
    entries = [(row, len(blob), mask, f.put(blob, 1)) for row, blob, mask in chunks]
    btree = _chunk_btree(f, entries, len(shape)) if entries else UNDEF
    layout = struct.pack("<BBBQ", 3, 2, len(shape) + 1, btree) + b"".join(struct.pack("<I", c) for c in chunk_shape)
    layout += struct.pack("<I", size)
    messages = [(0x1, _dataspace(shape, maxshape)), (0x3, _datatype(kind, size)), (0x5, bytes([2, 2, 0, 0]))]
    if filtered:
        name = b"lzf\0"
        messages.append((0xB, struct.pack("<BB6x", 1, 1) + struct.pack("<HHHH", 32000, len(name), 1, 3)
                         + name + b"\0" * 4 + struct.pack("<III", 4, 1, 0) + b"\0" * 4))
    messages.append((0x8, layout))
    return _object_header(f, messages, split)


def _small(f, kind, size, values, per_chunk, filtered=True):
    blob_rows = [values[k:k + per_chunk] for k in range(0, len(values), per_chunk)]
    chunks = []
    for k, rows in enumerate(blob_rows):
        full = np.zeros(per_chunk, dtype=values.dtype)
        full[:len(rows)] = rows
        raw = full.tobytes()
        chunks.append((k * per_chunk, lzf_compress(raw) if filtered else raw, 0 if filtered else 1))
    return _dataset(f, kind, size, (len(values),), (None,), (per_chunk,), chunks, filtered)


def chunk_rows_for(n_samples):
    """The reference's chunk shape (select.py:205)."""
    return max(1, int(1e6 / 4 / n_samples))


def encode_chunks(data, chunk_rows, raw=(), missing=(), cache=None):
    """(first row, stored blob, mask) per stored chunk of `data`; chunk numbers in `raw` are stored uncompressed
    (mask bit 0), those in `missing` are left out.  The last chunk is padded to full size with zeros."""
    out = []
    for k, row in enumerate(range(0, data.shape[0], chunk_rows)):
        if k in missing:
            continue
        full = np.zeros((chunk_rows,) + data.shape[1:], dtype=data.dtype)
        part = data[row:row + chunk_rows]
        full[:len(part)] = part
        raw_bytes = full.tobytes()
        if k in raw:
            out.append((row, raw_bytes, 1))
            continue
        blob = None if cache is None else cache.get(raw_bytes)
        if blob is None:
            blob = lzf_compress(raw_bytes)
            if cache is not None:
                cache[raw_bytes] = blob
        out.append((row, blob, 0) if len(blob) < len(raw_bytes) else (row, raw_bytes, 1))
    return out


def write_store(path, data=None, samples=None, var_count=None, chunk_rows=None, raw=(), missing=(), chunks=None,
                shape=None, dtype=None, split_headers=False):
    """Write a store.  Either `data` (n_var, n_samples) bool / float32, or already encoded `chunks` with `shape` and
    `dtype`.  var_count defaults to the column sums of data != 0."""
    if data is not None:
        shape, dtype = data.shape, data.dtype
    dtype = np.dtype(dtype)
    n_var, n_samples = shape
    chunk_rows = chunk_rows or chunk_rows_for(n_samples)
    if chunks is None:
        chunks = encode_chunks(data, chunk_rows, raw, missing)
    if samples is None:
        samples = [f"S{k:06d}" for k in range(n_samples)]
    if var_count is None:
        var_count = (data != 0).sum(axis=0) if data is not None else np.zeros(n_samples, np.int64)
    f = _File()
    kind = "bool" if dtype == np.bool_ else "float"
    data_at = _dataset(f, kind, dtype.itemsize, shape, (None, n_samples), (chunk_rows, n_samples), chunks,
                       split=split_headers)
    width = max(1, max(len(s) for s in samples))
    names = np.array([s.encode() for s in samples], dtype=f"S{width}")
    samples_at = _small(f, "string", width, names, 1250)
    vc_at = _small(f, "int", 8, np.asarray(var_count, dtype="<i8"), max(1, n_samples))
    # root group: local heap of names, one SNOD, a one-leaf group B-tree
    entries = sorted([("data", data_at), ("samples", samples_at), ("var_count", vc_at)])
    heap_data = bytearray(b"\0" * 8)
    offsets = []
    for name, _ in entries:
        offsets.append(len(heap_data))
        heap_data += name.encode() + b"\0"
        heap_data += b"\0" * (-len(heap_data) % 8)
    heap_data_at = f.put(bytes(heap_data))
    heap_at = f.put(b"HEAP" + struct.pack("<B3xQQQ", 0, len(heap_data), UNDEF, heap_data_at))
    snod = b"SNOD" + struct.pack("<BBH", 1, 0, len(entries))
    for (name, at), off in zip(entries, offsets):
        snod += struct.pack("<QQII16x", off, at, 0, 0)
    snod_at = f.put(snod)
    btree_at = f.put(b"TREE" + struct.pack("<BBHQQ", 0, 0, 1, UNDEF, UNDEF) + struct.pack("<QQQ", 0, snod_at, offsets[-1]))
    root_at = _object_header(f, [(0x11, struct.pack("<QQ", btree_at, heap_at))])
    eof = len(f.buf)
    sb = b"\x89HDF\r\n\x1a\n" + bytes([0, 0, 0, 0, 0, 8, 8, 0]) + struct.pack("<HHI", 4, 16, 0)
    sb += struct.pack("<QQQQ", 0, UNDEF, eof, UNDEF)
    sb += struct.pack("<QQII", 0, root_at, 1, 0) + struct.pack("<QQ", btree_at, heap_at)
    f.buf[:96] = sb
    with open(path, "wb") as fh:
        fh.write(f.buf)
    return path


def af_matrix(rng, n_var, n_samples, density=0.05, zero_rows=0):
    """float32 GT * AF: every row's carriers hold the row's AF; `zero_rows` rows hold nothing."""
    gt = rng.random((n_var, n_samples)) < density
    if zero_rows:
        gt[rng.choice(n_var, zero_rows, replace=False)] = False
    af = (rng.integers(1, 2 * n_samples, n_var) / (2 * n_samples)).astype(np.float32)
    return np.where(gt, af[:, None], np.float32(0)).astype(np.float32)
