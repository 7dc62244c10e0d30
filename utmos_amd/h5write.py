"""Writer of the reference's `--lowmem` HDF5 store (what `write_append_hdf5(is_first=True)` and then
`add_varcount_to_h5` write through h5py, utmos/select.py:198-238), byte for byte, without h5py.  h5store.py reads it.

The file is written as if by one write of its final contents.  For a store the reference writes in one dump (fewer
rows than its --buffer) the bytes are the reference's: tests/golden/h5/tiny.hdf5 and tiny.af.hdf5 are the
specification of every address, size and message below.  Layout (offsets of 8 bytes, lengths of 8 bytes):

    0        superblock, version 0 (96 B): group leaf K 4, internal K 16, end-of-file address, the root group's
             symbol-table entry (object header 96, cached B-tree 136 and local heap 680)
    96       root group object header (40 B): one symbol-table message
    136      root group B-tree (544 B): one leaf, one child (the SNOD), keys 0 and 24 (heap offset of "var_count")
    680      local heap (32 B) and its data (88 B at 712): "", "samples", "data", "var_count" at 0 / 8 / 16 / 24, one
             free block of 48 bytes at 40
    800      `samples` object header (16 + 256 B): dataspace (n,) max (unlimited,), string S{width} NUL-padded,
             fill value (v2, allocation incremental), filter pipeline (LZF, filter 32000, optional, client data
             4 / 0x105 / chunk bytes), layout v3 chunked, a NIL message up to 256 bytes
    1072     SNOD (328 B, room for 2 x leaf K entries): data, samples, var_count (sorted by name)
    1400     `samples` chunk B-tree (2,096 B: 64 entries of a rank-1 chunk key)
    3496     `samples` chunks, back to back
    ...      `data` object header (272 B): dataspace (rows, S) max (unlimited, S), bool enum FALSE / TRUE over int8
             or float32 LE, fill, LZF, layout (chunk_rows, S, itemsize)
    +272     `data` chunk B-tree (2,616 B: 64 entries of a rank-2 chunk key)
    +2,616   `data` chunks, back to back (the last one partial, stored full size)
    ...      `var_count` object header (272 B): int64 LE, dataspace (S,) max (S,); its chunk B-tree; its chunks
    EOF      the end of the last `var_count` chunk

Nothing is aligned (libhdf5 allocates at the end of the file).  A chunk is stored LZF-compressed when that fits in
the chunk's own size, else raw with filter-mask bit 0 set (h5py's filter gives liblzf an output buffer as long as the
chunk; no fixture holds a raw chunk).  The leaf's right-most key is what libhdf5's chunk B-tree leaves after inserting
chunks 0, 1, 2, ... in order: a chunk that lies at or past the right key moves it to the chunk's index + 1, the one
after it is inserted inside the key range, so the key is chunk_rows x (n if n is odd else n - 1) rows for n chunks;
the other dimensions hold their chunk extent.

Chunk shapes: `data` has max(1, int(1e6 / 4 / S)) rows of all S columns (select.py:205).  `samples` and `var_count`
are chunked by h5py's automatic rule (h5py's guess_chunk): the target size is 16 KiB x 2^log10(bytes / 1 MiB) clamped
to [8 KiB, 1 MiB], and the length is halved (rounding up) until the chunk is below the target, or within 50 % of it,
and below 1 MiB.  That gives 1,252 at 2,504 samples (S7 names and int64), the only size the fixtures pin.

Not pinned by any fixture, and so this build's choices: more than 64 chunks of a dataset (libhdf5 splits the B-tree
node as chunks arrive and allocates the new nodes between chunks; here the root stays where the single node would be,
and the levels below it follow the dataset's last chunk, every node full but the last of a level, with sibling
links); a store written by several dumps of the reference (--buffer rows each, each one a resize and a write, whose
allocation order cannot be checked here): the content -- shape, chunk shape, every chunk's cells and stored bytes,
samples, var_count -- is what such a file holds, the addresses are those of one write.
"""
import ctypes
import math
import struct

import numpy as np

UNDEF = 0xFFFFFFFFFFFFFFFF
SUPERBLOCK = 96
ROOT_HEADER = 96
ROOT_BTREE = 136
HEAP = 680
HEAP_DATA = 712
HEAP_DATA_SIZE = 88
SAMPLES_HEADER = 800
SNOD = 1072
SNOD_SIZE = 8 + 8 * 40
SAMPLES_BTREE = 1400
HEADER_SIZE = 16 + 256                 # every dataset's object header: prefix + 256 bytes of messages
FANOUT = 64                            # 2 x the chunk B-tree's K (32)
NAME_OFFSETS = {"samples": 8, "data": 16, "var_count": 24}
LZF_VERSION, H5PY_LZF_VERSION = 0x0105, 4


def data_chunk_rows(n_samples):
    """The reference's `data` chunk rows (select.py:205)."""
    return max(1, int(1e6 / 4 / n_samples))


def guess_chunk(length, itemsize):
    """h5py's automatic chunk length of a 1-D dataset (h5py's filters.guess_chunk)."""
    chunk = float(length if length else 1024)
    dset_size = chunk * itemsize
    target = 16 * 1024 * 2 ** math.log10(dset_size / (1024.0 * 1024))
    target = min(max(target, 8 * 1024), 1024 * 1024)
    while True:
        chunk_bytes = chunk * itemsize
        if (chunk_bytes < target or abs(chunk_bytes - target) / target < 0.5) and chunk_bytes < 1024 * 1024:
            break
        if chunk == 1:
            break
        chunk = math.ceil(chunk / 2.0)
    return int(chunk)


def btree_node_size(rank):
    return 24 + FANOUT * 8 + (FANOUT + 1) * (8 + 8 * (rank + 1))


def lzf_host(raw, out_cap=None):
    """utm_lzf_encode_host: the compressed chunk, or None when it does not fit in out_cap (default: the chunk's size)."""
    from . import _native as nat
    src = np.frombuffer(raw, dtype=np.uint8)
    cap = len(src) if out_cap is None else int(out_cap)
    out = np.empty(max(cap, 1), dtype=np.uint8)
    n = ctypes.c_uint64(0)
    nat.check(nat.lib().utm_lzf_encode_host(src.ctypes.data if len(src) else None, len(src), out.ctypes.data, cap,
                                            ctypes.byref(n)))
    return out[:n.value].tobytes() if n.value else None


def store_chunk(raw):
    """(stored bytes, filter mask) of one full-size chunk, as h5py's LZF filter stores it."""
    blob = lzf_host(raw)
    return (raw, 1) if blob is None else (blob, 0)


# ---------------------------------------------------------------------------------------------- messages
def _msg(mtype, body, flags):
    body = bytes(body) + b"\0" * (-len(body) % 8)
    return struct.pack("<HHB3x", mtype, len(body), flags) + body


def _object_header(messages):
    body = b"".join(_msg(t, b, f) for t, b, f in messages)
    assert len(body) + 8 <= 256
    body += struct.pack("<HHB3x", 0, 256 - len(body) - 8, 0) + b"\0" * (256 - len(body) - 8)
    return struct.pack("<BBHII4x", 1, 0, len(messages) + 1, 1, 256) + body


def _dataspace(shape, maxshape):
    return (struct.pack("<BBB5x", 1, len(shape), 1) + b"".join(struct.pack("<Q", d) for d in shape)
            + b"".join(struct.pack("<Q", d) for d in maxshape))


def _datatype(kind, size):
    if kind == "bool":        # h5py's bool: enum FALSE = 0, TRUE = 1 over a signed 8-bit integer
        base = bytes([0x10, 0x08, 0, 0]) + struct.pack("<IHH", 1, 0, 8)
        return bytes([0x18, 2, 0, 0]) + struct.pack("<I", 1) + base + b"FALSE\0\0\0TRUE\0\0\0\0" + bytes([0, 1])
    if kind == "float":
        return bytes([0x11, 0x20, 0x1F, 0]) + struct.pack("<IHHBBBBI", 4, 0, 32, 23, 8, 0, 23, 127)
    if kind == "int":         # signed little endian
        return bytes([0x10, 0x08, 0, 0]) + struct.pack("<IHH", size, 0, size * 8)
    if kind == "string":      # NUL-padded ASCII
        return bytes([0x13, 0x01, 0, 0]) + struct.pack("<I", size)
    raise ValueError(kind)


def _dataset_header(kind, itemsize, shape, maxshape, chunk_shape, btree):
    chunk_bytes = int(np.prod(chunk_shape)) * itemsize
    name = b"lzf\0\0\0\0\0"
    pipeline = (struct.pack("<BB6x", 1, 1) + struct.pack("<HHHH", 32000, 8, 1, 3) + name
                + struct.pack("<III4x", H5PY_LZF_VERSION, LZF_VERSION, chunk_bytes))
    layout = (struct.pack("<BBBQ", 3, 2, len(chunk_shape) + 1, btree)
              + b"".join(struct.pack("<I", c) for c in chunk_shape) + struct.pack("<I", itemsize))
    return _object_header([(0x1, _dataspace(shape, maxshape), 0), (0x3, _datatype(kind, itemsize), 1),
                           (0x5, bytes([2, 3, 0, 1, 0, 0, 0, 0]), 1), (0xB, pipeline, 1), (0x8, layout, 0)])


def _key(size, mask, row, chunk_shape):
    return struct.pack("<II", size, mask) + struct.pack(f"<{len(chunk_shape) + 1}Q", row, *([0] * len(chunk_shape)))


def _right_key(n_chunks, chunk_shape, itemsize):
    last = n_chunks if n_chunks % 2 else n_chunks - 1
    return struct.pack("<II", 0, 0) + struct.pack(f"<{len(chunk_shape) + 1}Q", last * chunk_shape[0],
                                                  *chunk_shape[1:], itemsize)


def _node(level, entries, right, rank, left_sib=UNDEF, right_sib=UNDEF):
    """entries: [(key, child address)] -> one full-size v1 B-tree node (type 1)."""
    body = b"".join(k + struct.pack("<Q", a) for k, a in entries) + right
    blob = b"TREE" + struct.pack("<BBHQQ", 1, level, len(entries), left_sib, right_sib) + body
    return blob + b"\0" * (btree_node_size(rank) - len(blob))


def chunk_btree(table, chunk_shape, itemsize, root_at, end_at):
    """table: [(row, stored size, mask, address)] in row order -> (root node bytes, [lower nodes]); the root goes at
    root_at, the lower nodes (more than 64 chunks) back to back from end_at."""
    rank = len(chunk_shape)
    size = btree_node_size(rank)
    right = _right_key(len(table), chunk_shape, itemsize)
    level = [(_key(s, m, r, chunk_shape), a) for r, s, m, a in table]
    depth = 0
    lower, at = [], end_at
    while len(level) > FANOUT:                    # cut into full nodes; each becomes one entry of the level above
        groups = [level[k:k + FANOUT] for k in range(0, len(level), FANOUT)]
        addrs = [at + k * size for k in range(len(groups))]
        up = []
        for k, g in enumerate(groups):
            rk = groups[k + 1][0][0] if k + 1 < len(groups) else right
            lower.append(_node(depth, g, rk, rank, addrs[k - 1] if k else UNDEF,
                               addrs[k + 1] if k + 1 < len(groups) else UNDEF))
            up.append((g[0][0], addrs[k]))
        at += len(groups) * size
        level = up
        depth += 1
    return _node(depth, level, right, rank), lower


# ---------------------------------------------------------------------------------------------- encoders
class HostChunkEncoder:
    """`data` chunks on the CPU: cells by numpy, LZF by utm_lzf_encode_host (the device's bytes)."""

    def __init__(self, chunk_rows, n_cols, itemsize):
        self.chunk_rows, self.n_cols, self.itemsize = chunk_rows, n_cols, itemsize
        self.batch_rows = chunk_rows * max(1, (64 << 20) // (chunk_rows * n_cols * itemsize))
        self.done = []

    def submit(self, rows, af):
        gt = np.unpackbits(rows, axis=1, count=self.n_cols)
        cells = gt.astype(bool) if self.itemsize == 1 else gt.astype(np.float32) * np.asarray(af, np.float32)[:, None]
        blobs, sizes, masks = [], [], []
        for lo in range(0, len(rows), self.chunk_rows):
            full = np.zeros((self.chunk_rows, self.n_cols), cells.dtype)
            part = cells[lo:lo + self.chunk_rows]
            full[:len(part)] = part
            blob, mask = store_chunk(full.tobytes())
            blobs.append(blob)
            sizes.append(len(blob))
            masks.append(mask)
        self.done.append((b"".join(blobs), sizes, masks))

    def results(self, final=False):
        out, self.done = self.done, []
        return out

    def close(self):
        pass


class GpuChunkEncoder:
    """`data` chunks on a GPU (utm_h5w_*): two batches in flight, so the host writes one batch's chunks while the
    device encodes the next."""

    def __init__(self, chunk_rows, n_cols, itemsize, device=0, max_chunks=None):
        from . import _native as nat
        self.nat = nat
        self.chunk_rows, self.n_cols, self.itemsize = chunk_rows, n_cols, itemsize
        chunk_bytes = chunk_rows * n_cols * itemsize
        if max_chunks is None:
            max_chunks = max(1, min(4096, (256 << 20) // chunk_bytes))
        self.max_chunks = int(max_chunks)
        self.batch_rows = self.max_chunks * chunk_rows
        self.h = ctypes.c_void_p()
        nat.check(nat.lib().utm_h5w_create(int(device), chunk_rows, n_cols, itemsize, self.max_chunks,
                                           ctypes.byref(self.h)))
        self.inflight = 0
        self.sizes = np.zeros(self.max_chunks, np.uint32)
        self.masks = np.zeros(self.max_chunks, np.uint32)

    def submit(self, rows, af):
        rows = np.ascontiguousarray(rows, dtype=np.uint8)
        af = None if self.itemsize == 1 else np.ascontiguousarray(af, dtype=np.float32)
        self.nat.check(self.nat.lib().utm_h5w_encode(self.h, rows.ctypes.data, None if af is None else af.ctypes.data,
                                                     len(rows)))
        self.inflight += 1

    def _fetch(self):
        out, n_bytes, n = ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_uint32()
        self.nat.check(self.nat.lib().utm_h5w_fetch(self.h, ctypes.byref(out), ctypes.byref(n_bytes),
                                                    self.sizes.ctypes.data, self.masks.ctypes.data, ctypes.byref(n)))
        self.inflight -= 1
        blob = ctypes.string_at(out.value, n_bytes.value) if n_bytes.value else b""
        return blob, self.sizes[:n.value].tolist(), self.masks[:n.value].tolist()

    def results(self, final=False):
        """Fetched batches: the oldest once two are queued, all of them when final."""
        out = []
        while self.inflight >= (1 if final else 2):
            out.append(self._fetch())
        return out

    def timing(self):
        ms = (ctypes.c_double * 4)()
        self.nat.check(self.nat.lib().utm_h5w_timing(self.h, ms))
        return dict(zip(("h2d", "cells", "encode", "d2h"), list(ms)))

    def close(self):
        if self.h:
            self.nat.lib().utm_h5w_destroy(self.h)
            self.h = ctypes.c_void_p()


# ---------------------------------------------------------------------------------------------- the file
class H5Writer:
    """with H5Writer(path, samples, with_af, encoder) as w: w.add_rows(packbits rows, af32) ...; w.finish(var_count).
    Rows arrive in any pieces; whole chunks go to the encoder in batches and their stored bytes to the file as they
    come back, so the host holds at most a batch of rows and two batches of chunks."""

    def __init__(self, path, samples, with_af, encoder="gpu", device=0, max_chunks=None):
        self.path = path
        names = [str(s).encode("utf-8") for s in samples]
        self.n_samples = len(names)
        self.itemsize = 4 if with_af else 1
        self.chunk_rows = data_chunk_rows(self.n_samples)
        if encoder == "gpu":
            encoder = GpuChunkEncoder(self.chunk_rows, self.n_samples, self.itemsize, device, max_chunks)
        elif encoder == "host":
            encoder = HostChunkEncoder(self.chunk_rows, self.n_samples, self.itemsize)
        self.enc = encoder
        self.row_bytes = (self.n_samples + 7) // 8
        self.pending_rows = np.empty((0, self.row_bytes), np.uint8)
        self.pending_af = np.empty(0, np.float32)
        self.n_rows = 0
        self.table = []                           # (row, stored size, mask, address) per `data` chunk
        self.fh = open(path, "wb")
        self.done = False
        # samples: known now, so everything up to the `data` chunks is laid out at once
        width = max([1] + [len(n) for n in names])
        cells = np.array(names, dtype=f"S{width}") if names else np.zeros(0, f"S{width}")
        s_chunk = guess_chunk(self.n_samples, width)
        s_table, s_blobs, at = [], [], SAMPLES_BTREE + btree_node_size(1)
        for k, row in enumerate(range(0, self.n_samples, s_chunk)):
            full = np.zeros(s_chunk, f"S{width}")
            part = cells[row:row + s_chunk]
            full[:len(part)] = part
            blob, mask = store_chunk(full.tobytes())
            s_table.append((row, len(blob), mask, at))
            s_blobs.append(blob)
            at += len(blob)
        s_root, s_lower = chunk_btree(s_table, (s_chunk,), width, SAMPLES_BTREE, at)
        at += sum(len(n) for n in s_lower)
        self.data_header = at
        self.data_btree = at + HEADER_SIZE
        self.at = self.data_btree + btree_node_size(2)
        self.fh.write(b"\0" * SAMPLES_HEADER)     # superblock, root group and heap: written by finish
        self.fh.write(_dataset_header("string", width, (self.n_samples,), (UNDEF,), (s_chunk,),
                                      SAMPLES_BTREE if s_table else UNDEF))
        self.fh.write(b"\0" * SNOD_SIZE)
        self.fh.write(s_root if s_table else b"\0" * btree_node_size(1))
        for blob in s_blobs + s_lower:
            self.fh.write(blob)
        self.fh.write(b"\0" * (self.at - self.fh.tell()))   # `data` header and B-tree root: written by finish

    # --------------------------------------------------------------------------------------- rows
    def add_rows(self, rows, af=None):
        """packbits rows (n, ceil(S / 8)) uint8 in numpy order; af: float32 (n,) for an AF store."""
        rows = np.asarray(rows, dtype=np.uint8).reshape(-1, self.row_bytes)
        if self.itemsize == 4:
            if af is None or len(af) != len(rows):
                raise ValueError("an AF store needs one AF value per row")
            self.pending_af = np.concatenate([self.pending_af, np.asarray(af, dtype=np.float32)])
        self.pending_rows = np.concatenate([self.pending_rows, rows]) if len(self.pending_rows) else rows
        self.n_rows += len(rows)
        while len(self.pending_rows) >= self.enc.batch_rows:
            self._submit(self.enc.batch_rows)

    def _submit(self, n):
        self.enc.submit(self.pending_rows[:n], self.pending_af[:n] if self.itemsize == 4 else None)
        self.pending_rows = self.pending_rows[n:]
        self.pending_af = self.pending_af[n:]
        self._write(self.enc.results())

    def _write(self, batches):
        for blob, sizes, masks in batches:
            self.fh.seek(self.at)
            self.fh.write(blob)
            for size, mask in zip(sizes, masks):
                self.table.append((len(self.table) * self.chunk_rows, int(size), int(mask), self.at))
                self.at += int(size)

    # --------------------------------------------------------------------------------------- the rest
    def finish(self, var_count):
        if len(self.pending_rows):
            self._submit(len(self.pending_rows))
        self._write(self.enc.results(final=True))
        self.enc.close()
        fh = self.fh
        d_root, d_lower = chunk_btree(self.table, (self.chunk_rows, self.n_samples), self.itemsize, self.data_btree,
                                      self.at)
        fh.seek(self.at)
        for node in d_lower:
            fh.write(node)
        vc_header = fh.tell()
        vc = np.asarray(var_count, dtype="<i8").reshape(-1)
        if len(vc) != self.n_samples:
            raise ValueError(f"{len(vc)} var_count values for {self.n_samples} samples")
        v_chunk = guess_chunk(self.n_samples, 8)
        v_btree = vc_header + HEADER_SIZE
        at = v_btree + btree_node_size(1)
        v_table, v_blobs = [], []
        for row in range(0, self.n_samples, v_chunk):
            full = np.zeros(v_chunk, "<i8")
            part = vc[row:row + v_chunk]
            full[:len(part)] = part
            blob, mask = store_chunk(full.tobytes())
            v_table.append((row, len(blob), mask, at))
            v_blobs.append(blob)
            at += len(blob)
        v_root, v_lower = chunk_btree(v_table, (v_chunk,), 8, v_btree, at)
        fh.write(_dataset_header("int", 8, (self.n_samples,), (self.n_samples,), (v_chunk,),
                                 v_btree if v_table else UNDEF))
        fh.write(v_root if v_table else b"\0" * btree_node_size(1))
        for blob in v_blobs + v_lower:
            fh.write(blob)
        eof = fh.tell()
        # the `data` header and B-tree root, now that the rows are counted
        fh.seek(self.data_header)
        kind = "float" if self.itemsize == 4 else "bool"
        fh.write(_dataset_header(kind, self.itemsize, (self.n_rows, self.n_samples), (UNDEF, self.n_samples),
                                 (self.chunk_rows, self.n_samples), self.data_btree if self.table else UNDEF))
        fh.write(d_root if self.table else b"\0" * btree_node_size(2))
        # superblock, root group, local heap, SNOD
        fh.seek(0)
        sb = b"\x89HDF\r\n\x1a\n" + bytes([0, 0, 0, 0, 0, 8, 8, 0]) + struct.pack("<HHI", 4, 16, 0)
        sb += struct.pack("<QQQQ", 0, UNDEF, eof, UNDEF)
        sb += struct.pack("<QQII", 0, ROOT_HEADER, 1, 0) + struct.pack("<QQ", ROOT_BTREE, HEAP)
        root = struct.pack("<BBHII4x", 1, 0, 1, 1, 24) + _msg(0x11, struct.pack("<QQ", ROOT_BTREE, HEAP), 0)
        gtree = b"TREE" + struct.pack("<BBHQQ", 0, 0, 1, UNDEF, UNDEF) + struct.pack("<QQQ", 0, SNOD, 24)
        gtree += b"\0" * (HEAP - ROOT_BTREE - len(gtree))
        heap = b"HEAP" + struct.pack("<B3xQQQ", 0, HEAP_DATA_SIZE, 40, HEAP_DATA)
        names = b"\0" * 8 + b"samples\0" + b"data\0\0\0\0" + b"var_count\0\0\0\0\0\0\0" + struct.pack("<QQ", 1, 48)
        names += b"\0" * (HEAP_DATA_SIZE - len(names))
        fh.write(sb + root + gtree + heap + names)
        assert fh.tell() == SAMPLES_HEADER
        fh.seek(SNOD)
        snod = b"SNOD" + struct.pack("<BBH", 1, 0, 3)
        for name, addr in (("data", self.data_header), ("samples", SAMPLES_HEADER), ("var_count", vc_header)):
            snod += struct.pack("<QQII16x", NAME_OFFSETS[name], addr, 0, 0)
        fh.write(snod + b"\0" * (SNOD_SIZE - len(snod)))
        fh.close()
        self.done = True

    def close(self):
        if not self.done:
            self.enc.close()
            self.fh.close()
            self.done = True

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
