"""Read-only reader of the reference's `--lowmem` HDF5 store (utmos/select.py:198-238, written by h5py), for exactly
the subset of HDF5 that h5py writes there:

    superblock version 0 (or 1), the root group a symbol table (v1 group B-tree -> SNOD nodes, local heap for the
    names), v1 object headers (continuation messages followed); datasets chunked (layout message v3, chunks indexed by
    a v1 B-tree of type 1) or contiguous, filter pipeline empty or LZF (h5py's filter 32000), fill value zero.

    data       (n_var, n_samples) bool enum over int8 (or int8 / uint8), or float32 LE (GT * AF, written with --af);
               chunks of whole rows, the last one partial but stored full size
    samples    fixed-length byte strings, NUL padded
    var_count  int64 per sample, from the boolean GT (select.py:233-238, :280-284)

Anything outside the subset is a ValueError that names it.  Only the structure and the two small datasets are read
here (their LZF chunks through utm_lzf_decode_host); the `data` chunks are decoded and packed on the GPU
(`ChunkDecoder`, csrc/lzf.hip.h).  No h5py.
"""
import ctypes
import struct

import numpy as np

SIGNATURE = b"\x89HDF\r\n\x1a\n"
UNDEF = 0xFFFFFFFFFFFFFFFF
LZF_FILTER = 32000
LZF_ERRORS = {1: "an LZF token runs past the chunk's stored bytes", 2: "more output than the chunk holds",
              3: "less output than the chunk holds", 4: "an LZF back-reference before the start of the chunk",
              5: "a row whose nonzero float32 values differ, or are negative or NaN"}


class Dataset:
    """One dataset's shape, type and storage: `chunks` = [(first row, file offset, stored bytes, filter mask)] by row."""

    def __init__(self, name):
        self.name = name
        self.shape = None
        self.dtype = None          # numpy dtype of the cells
        self.kind = None           # "bool", "int", "float" or "string"
        self.chunk_shape = None
        self.filtered = False      # LZF in the pipeline (else every chunk is stored raw)
        self.contiguous = None     # (file offset, bytes) of a contiguous dataset
        self.btree = None
        self.chunks = []

    @property
    def itemsize(self):
        return self.dtype.itemsize

    @property
    def chunk_rows(self):
        return self.chunk_shape[0]

    @property
    def chunk_bytes(self):
        return int(np.prod(self.chunk_shape)) * self.itemsize


class H5Store:
    """H5Store(path): .samples (str), .var_count (int64), .data (Dataset: shape, dtype, chunk_rows, chunks)."""

    def __init__(self, path):
        self.path = path
        with open(path, "rb") as fh:
            self.fh = fh
            self._parse()
        self.fh = None

    # ------------------------------------------------------------------------------------------ raw access
    def _read(self, offset, size):
        self.fh.seek(offset)
        blob = self.fh.read(size)
        if len(blob) != size:
            raise ValueError(f"{self.path}: truncated at byte {offset} (+{size})")
        return blob

    def _addr(self, blob, at):
        return int.from_bytes(blob[at:at + self.so], "little")

    def _len(self, blob, at):
        return int.from_bytes(blob[at:at + self.sl], "little")

    # ------------------------------------------------------------------------------------------ structure
    def _parse(self):
        head = self._read(0, 24)
        if head[:8] != SIGNATURE:
            raise ValueError(f"{self.path}: not an HDF5 file (no signature at byte 0)")
        version = head[8]
        if version not in (0, 1):
            raise ValueError(f"{self.path}: HDF5 superblock version {version} (this reader takes 0 and 1)")
        self.so, self.sl = head[13], head[14]
        if self.so not in (4, 8) or self.sl not in (4, 8):
            raise ValueError(f"{self.path}: offsets of {self.so} and lengths of {self.sl} bytes")
        at = 24 + (4 if version == 1 else 0)            # v1: indexed storage K and a reserved word
        rest = self._read(at, 4 * self.so + 2 * self.so + 24)
        if self._addr(rest, 0) != 0:
            raise ValueError(f"{self.path}: base address {self._addr(rest, 0)} (only 0 is read)")
        entry = rest[4 * self.so:]                        # root group symbol table entry
        header = self._addr(entry, self.so)
        cache = struct.unpack_from("<I", entry, 2 * self.so)[0]
        if cache == 1:
            btree, heap = self._addr(entry, 2 * self.so + 8), self._addr(entry, 3 * self.so + 8)
        else:
            msgs = self._messages(header)
            if 0x11 not in msgs:
                raise ValueError(f"{self.path}: the root group is not a symbol table (only v0 / v1 groups are read)")
            body = msgs[0x11]
            btree, heap = self._addr(body, 0), self._addr(body, self.so)
        names = self._group(btree, heap)
        for need in ("data", "samples", "var_count"):
            if need not in names:
                raise ValueError(f"{self.path}: no `{need}` dataset in the root group (found {sorted(names)})")
        self.data = self._dataset("data", names["data"])
        if len(self.data.shape) != 2:
            raise ValueError(f"{self.path}: `data` has {len(self.data.shape)} dimensions, expected 2")
        if self.data.kind not in ("bool", "int", "float") or self.data.itemsize not in (1, 4) or \
                (self.data.kind == "float") != (self.data.itemsize == 4):
            raise ValueError(f"{self.path}: `data` cells of type {self.data.kind}{self.data.itemsize * 8}: "
                             "expected bool, int8, uint8 or float32")
        if self.data.chunk_shape is not None and self.data.chunk_shape[1] != self.data.shape[1]:
            raise ValueError(f"{self.path}: `data` chunks of {self.data.chunk_shape[1]} columns do not span the "
                             f"{self.data.shape[1]} columns")
        samples = self._dataset("samples", names["samples"])
        if samples.kind != "string":
            raise ValueError(f"{self.path}: `samples` are not fixed-length strings")
        raw = self.read_small(samples)
        self.samples = np.array([s.rstrip(b"\0").decode("utf-8") for s in raw.tolist()], dtype=str)
        var_count = self._dataset("var_count", names["var_count"])
        if var_count.kind != "int":
            raise ValueError(f"{self.path}: `var_count` is not an integer dataset")
        self.var_count = self.read_small(var_count).astype(np.int64)
        if len(self.samples) != self.data.shape[1] or len(self.var_count) != self.data.shape[1]:
            raise ValueError(f"{self.path}: {len(self.samples)} samples and {len(self.var_count)} var_count values "
                             f"for {self.data.shape[1]} columns")

    def _group(self, btree, heap):
        """{name: object header address} of a v1 symbol-table group."""
        h = self._read(heap, 8 + 2 * self.sl + self.so)
        if h[:4] != b"HEAP":
            raise ValueError(f"{self.path}: no local heap at byte {heap}")
        heap_size, heap_data = self._len(h, 8), self._addr(h, 8 + 2 * self.sl)
        names_blob = self._read(heap_data, heap_size)
        out = {}
        for snod in self._btree(btree, 0):
            s = self._read(snod, 8)
            if s[:4] != b"SNOD":
                raise ValueError(f"{self.path}: no symbol table node at byte {snod}")
            count = struct.unpack_from("<H", s, 6)[0]
            size = 2 * self.so + 24
            entries = self._read(snod + 8, count * size)
            for k in range(count):
                e = entries[k * size:(k + 1) * size]
                name_off = self._len(e, 0)
                end = names_blob.index(b"\0", name_off)
                out[names_blob[name_off:end].decode("utf-8")] = self._addr(e, self.so)
        return out

    def _btree(self, address, node_type, rank=0):
        """Children of a v1 B-tree in key order.  Type 0 (group): SNOD addresses.  Type 1 (chunks): (key, address)
        with key = (stored bytes, filter mask, offsets...)."""
        key_size = self.sl if node_type == 0 else 8 + 8 * (rank + 1)
        out = []
        todo = [address]
        while todo:
            node = todo.pop(0)
            h = self._read(node, 8 + 2 * self.so)
            if h[:4] != b"TREE":
                raise ValueError(f"{self.path}: no B-tree node at byte {node}")
            if h[4] != node_type:
                raise ValueError(f"{self.path}: B-tree node of type {h[4]} where type {node_type} was expected")
            level, used = h[5], struct.unpack_from("<H", h, 6)[0]
            body = self._read(node + 8 + 2 * self.so, used * (key_size + self.so) + key_size)
            children = []
            for k in range(used):
                at = k * (key_size + self.so)
                key = body[at:at + key_size]
                child = self._addr(body, at + key_size)
                if level > 0:
                    children.append(child)
                elif node_type == 0:
                    out.append(child)
                else:
                    size, mask = struct.unpack_from("<II", key, 0)
                    offsets = struct.unpack_from(f"<{rank + 1}Q", key, 8)
                    out.append(((size, mask) + offsets, child))
            todo = children + todo                          # depth first keeps the key order
        return out

    def _messages(self, address):
        """{type: body} of a v1 object header, continuation blocks followed (the first message of a type wins)."""
        h = self._read(address, 16)
        if h[:4] == b"OHDR":
            raise ValueError(f"{self.path}: version 2 object header at byte {address} (only version 1 is read)")
        if h[0] != 1:
            raise ValueError(f"{self.path}: object header version {h[0]} at byte {address}")
        n_msgs = struct.unpack_from("<H", h, 2)[0]
        size = struct.unpack_from("<I", h, 8)[0]
        blocks = [(address + 16, size)]
        msgs = {}
        seen = 0
        while blocks and seen < n_msgs:
            start, length = blocks.pop(0)
            blob = self._read(start, length)
            at = 0
            while at + 8 <= length and seen < n_msgs:
                mtype, msize, flags = struct.unpack_from("<HHB", blob, at)
                body = blob[at + 8:at + 8 + msize]
                at += 8 + msize
                seen += 1
                if flags & 0x02:
                    raise ValueError(f"{self.path}: shared object header message (type {mtype}) at byte {address}")
                if mtype == 0x10:
                    blocks.append((self._addr(body, 0), self._len(body, self.so)))
                elif mtype not in msgs:
                    msgs[mtype] = body
        return msgs

    def _datatype(self, body, ds):
        cls, version = body[0] & 0x0F, body[0] >> 4
        bits = body[1] | body[2] << 8 | body[3] << 16
        size = struct.unpack_from("<I", body, 4)[0]
        if cls == 0:
            if bits & 1:
                raise ValueError(f"{self.path}: `{ds.name}` is big endian")
            ds.kind = "int"
            ds.dtype = np.dtype(f"<{'i' if bits & 8 else 'u'}{size}")
        elif cls == 1:
            if bits & 1 or size != 4:
                raise ValueError(f"{self.path}: `{ds.name}` is a {size * 8}-bit{' big-endian' if bits & 1 else ''} float")
            ds.kind, ds.dtype = "float", np.dtype("<f4")
        elif cls == 3:
            ds.kind, ds.dtype = "string", np.dtype(f"S{size}")
        elif cls == 8:                                     # enum: h5py's bool is FALSE = 0, TRUE = 1 over int8
            base = body[8:]
            if base[0] & 0x0F != 0 or struct.unpack_from("<I", base, 4)[0] != 1:
                raise ValueError(f"{self.path}: `{ds.name}` is an enum over a base type other than a 1-byte integer")
            n = bits & 0xFFFF
            at = 8 + 12                                   # the base type: 8 bytes + 4 bytes of integer properties
            names = []
            for _ in range(n):
                end = body.index(b"\0", at)
                names.append(body[at:end].decode("ascii", "replace"))
                at = end + 1 if version >= 3 else at + ((end - at) // 8 + 1) * 8
            values = list(body[at:at + n])
            if dict(zip(names, values)) != {"FALSE": 0, "TRUE": 1}:
                raise ValueError(f"{self.path}: `{ds.name}` is an enum {dict(zip(names, values))}, not h5py's bool")
            ds.kind, ds.dtype = "bool", np.dtype("u1")
        else:
            raise ValueError(f"{self.path}: `{ds.name}` has datatype class {cls}")

    def _dataset(self, name, address):
        ds = Dataset(name)
        msgs = self._messages(address)
        for need, what in ((0x1, "dataspace"), (0x3, "datatype"), (0x8, "layout")):
            if need not in msgs:
                raise ValueError(f"{self.path}: `{name}` has no {what} message")
        body = msgs[0x1]
        version, rank, flags = body[0], body[1], body[2]
        at = 8 if version == 1 else 4
        ds.shape = tuple(self._len(body, at + k * self.sl) for k in range(rank))
        self._datatype(msgs[0x3], ds)
        for fill_type in (0x5, 0x4):
            if fill_type in msgs:
                self._check_fill(msgs[fill_type], fill_type, ds)
        if 0xB in msgs:
            self._filters(msgs[0xB], ds)
        layout = msgs[0x8]
        if layout[0] != 3:
            raise ValueError(f"{self.path}: `{name}` has a version {layout[0]} layout message (only version 3 is read)")
        if layout[1] == 1:
            ds.contiguous = (self._addr(layout, 2), self._len(layout, 2 + self.so))
        elif layout[1] == 2:
            dims = layout[2]
            ds.btree = self._addr(layout, 3)
            shape = struct.unpack_from(f"<{dims}I", layout, 3 + self.so)
            if dims != rank + 1 or shape[-1] != ds.itemsize:
                raise ValueError(f"{self.path}: `{name}` chunk dimensions {shape} for a rank-{rank} dataset")
            ds.chunk_shape = tuple(int(x) for x in shape[:-1])
            ds.chunks = self._chunk_table(ds, rank)
        else:
            raise ValueError(f"{self.path}: `{name}` has layout class {layout[1]} (chunked and contiguous are read)")
        return ds

    def _check_fill(self, body, mtype, ds):
        """Only the default fill value, zero, is read."""
        if mtype == 0x4:
            size, value = struct.unpack_from("<I", body, 0)[0], body[4:]
        elif body[0] in (1, 2):
            defined = body[3]
            if body[0] == 2 and not defined:
                return
            size = struct.unpack_from("<I", body, 4)[0]
            value = body[8:8 + size]
        elif body[0] == 3:
            if not body[1] & 0x20:
                return
            size = struct.unpack_from("<I", body, 2)[0]
            value = body[6:6 + size]
        else:
            raise ValueError(f"{self.path}: `{ds.name}` has a version {body[0]} fill value message")
        if size and any(value[:size]):
            raise ValueError(f"{self.path}: `{ds.name}` has a fill value other than zero")

    def _filters(self, body, ds):
        version, n = body[0], body[1]
        at = 8 if version == 1 else 2
        for _ in range(n):
            fid = struct.unpack_from("<H", body, at)[0]
            if version == 1 or fid >= 256:
                name_len = struct.unpack_from("<H", body, at + 2)[0]
                at += 4
            else:
                name_len = 0
                at += 2
            _flags, n_values = struct.unpack_from("<HH", body, at)
            at += 4
            if version == 1:
                at += (name_len + 7) // 8 * 8 + 4 * n_values + (4 if n_values % 2 else 0)
            else:
                at += name_len + 4 * n_values
            if fid != LZF_FILTER:
                raise ValueError(f"{self.path}: `{ds.name}` uses filter {fid} (only LZF, {LZF_FILTER}, is read)")
            ds.filtered = True

    def _chunk_table(self, ds, rank):
        table = []
        if ds.btree != UNDEF:
            for key, child in self._btree(ds.btree, 1, rank):
                size, mask, offsets = key[0], key[1], key[2:]
                if any(offsets[1:]):
                    raise ValueError(f"{self.path}: `{ds.name}` has a chunk at column {offsets[1]}: chunks must span "
                                     "all columns")
                table.append((int(offsets[0]), int(child), int(size), int(mask) if ds.filtered else 1))
        table.sort()
        return table

    # ------------------------------------------------------------------------------------------ small datasets
    def read_small(self, ds):
        """The whole dataset as a numpy array, decoded on the host (for `samples` and `var_count`)."""
        n = ds.shape[0] if ds.shape else 1
        cells = int(np.prod(ds.shape[1:])) if len(ds.shape) > 1 else 1
        out = np.zeros(n * cells * ds.itemsize, dtype=np.uint8)
        with open(self.path, "rb") as fh:
            if ds.contiguous is not None:
                fh.seek(ds.contiguous[0])
                blob = fh.read(min(ds.contiguous[1], len(out)))
                out[:len(blob)] = np.frombuffer(blob, dtype=np.uint8)
            else:
                row_bytes = cells * ds.itemsize
                for row, offset, size, mask in ds.chunks:
                    fh.seek(offset)
                    stored = fh.read(size)
                    chunk = stored if mask & 1 else lzf_decode(stored, ds.chunk_bytes, f"{self.path}: `{ds.name}` "
                                                                                      f"chunk at row {row}")
                    take = min(ds.chunk_rows, n - row) * row_bytes
                    out[row * row_bytes:row * row_bytes + take] = np.frombuffer(chunk, dtype=np.uint8)[:take]
        return out.view(ds.dtype).reshape(ds.shape)


def lzf_decode(stored, n_out, what="LZF chunk"):
    """One LZF chunk -> exactly n_out bytes, by utm_lzf_decode_host (the device decoder's parser on the CPU)."""
    from . import _native as nat
    out = np.empty(n_out, dtype=np.uint8)
    src = np.frombuffer(stored, dtype=np.uint8)
    status = ctypes.c_uint32(0)
    nat.check(nat.lib().utm_lzf_decode_host(src.ctypes.data if len(src) else None, len(src),
                                            out.ctypes.data if n_out else None, n_out, ctypes.byref(status)))
    if status.value:
        raise ValueError(f"{what}: {LZF_ERRORS.get(status.value, f'status {status.value}')}")
    return out.tobytes()


class ChunkDecoder:
    """The `data` chunks of a store, decoded and packed on a GPU (utm_h5_*), in batches: iterate to get
    (first row, packbits rows uint8 (n, ceil(S/8)), af float32 (n,) or None).  Two batches are in flight: the next
    batch is read from the file into the pinned staging while the device decodes the last one."""

    def __init__(self, store, device=0, stage_bytes=256 << 20, max_chunks=None):
        from . import _native as nat
        self.nat = nat
        self.store, self.ds = store, store.data
        ds = self.ds
        self.n_var, self.n_cols = ds.shape
        if ds.contiguous is not None:                  # contiguous data: raw pseudo-chunks of whole rows
            row_bytes = self.n_cols * ds.itemsize
            self.chunk_rows = max(1, min(self.n_var, (1 << 20) // max(1, row_bytes)))
            self.chunks = [(r, ds.contiguous[0] + r * row_bytes, self.chunk_rows * row_bytes, 1)
                           for r in range(0, self.n_var, self.chunk_rows)]
            self.file_end = ds.contiguous[0] + self.n_var * row_bytes     # the last one is read up to here, zero padded
        else:
            self.chunk_rows = ds.chunk_rows
            self.chunks = list(ds.chunks)
            self.file_end = None
        chunk_bytes = self.chunk_rows * self.n_cols * ds.itemsize
        largest = max([c[2] for c in self.chunks if c] + [chunk_bytes])
        self.stage_bytes = int(max(stage_bytes, largest))
        if max_chunks is None:
            max_chunks = max(1, min(4096, (512 << 20) // max(1, chunk_bytes)))
        self.max_chunks = int(max_chunks)
        self.row_bytes = (self.n_cols + 7) // 8
        self.h = ctypes.c_void_p()
        nat.check(nat.lib().utm_h5_create(int(device), self.stage_bytes, self.max_chunks, self.chunk_rows,
                                          self.n_cols, ds.itemsize, ctypes.byref(self.h)))
        buf, cap = ctypes.c_void_p(), ctypes.c_uint64()
        nat.check(nat.lib().utm_h5_staging(self.h, ctypes.byref(buf), ctypes.byref(cap)))
        self.stage = np.ctypeslib.as_array(ctypes.cast(buf, ctypes.POINTER(ctypes.c_uint8)), shape=(cap.value,))

    def close(self):
        if self.h:
            self.nat.lib().utm_h5_destroy(self.h)
            self.h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def timing(self):
        """HIP-event milliseconds summed over the fetched batches: h2d, decode, pack, d2h."""
        ms = (ctypes.c_double * 4)()
        self.nat.check(self.nat.lib().utm_h5_timing(self.h, ms))
        return dict(zip(("h2d", "decode", "pack", "d2h"), list(ms)))

    def _plan(self):
        """Chunks in row order, absent ones filled in, cut into batches that fit the staging and max_chunks."""
        step = self.chunk_rows
        have = {c[0]: c for c in self.chunks if c}
        batch, stored = [], 0
        for row in range(0, self.n_var, step):
            c = have.get(row, (row, 0, 0, 0))
            if batch and (len(batch) == self.max_chunks or stored + c[2] > self.stage_bytes):
                yield batch
                batch, stored = [], 0
            batch.append(c)
            stored += c[2]
        if batch:
            yield batch

    def _submit(self, fh, batch):
        n = len(batch)
        offsets = np.zeros(n, np.uint64)
        sizes = np.array([c[2] for c in batch], np.uint64)
        masks = np.array([c[3] for c in batch], np.uint32)
        rows = np.array([min(self.chunk_rows, self.n_var - c[0]) for c in batch], np.uint32)
        at = 0
        k = 0
        while k < n:                                    # one read per run of chunks that follow each other in the file
            j, end = k, batch[k][1] + batch[k][2]
            while j + 1 < n and batch[j + 1][2] and batch[j + 1][1] == end:
                j += 1
                end += batch[j][2]
            length = end - batch[k][1]
            if length:
                fh.seek(batch[k][1])
                want = length if self.file_end is None else min(length, self.file_end - batch[k][1])
                got = fh.readinto(memoryview(self.stage[at:at + want]))
                self.stage[at + want:at + length] = 0
                if got != want:
                    raise ValueError(f"{self.store.path}: truncated `data` chunk at row {batch[k][0]}")
            for m in range(k, j + 1):
                offsets[m] = at
                at += batch[m][2]
            k = j + 1
        self.nat.check(self.nat.lib().utm_h5_decode(self.h, self.stage.ctypes.data, at, offsets.ctypes.data,
                                                    sizes.ctypes.data, masks.ctypes.data, rows.ctypes.data, n))
        return batch, int(rows.sum())

    def _fetch(self, batch, n_rows):
        packed = np.empty((n_rows, self.row_bytes), np.uint8)
        af = np.empty(n_rows, np.float32) if self.ds.itemsize == 4 else None
        status = np.zeros(len(batch), np.uint32)
        self.nat.check(self.nat.lib().utm_h5_fetch(self.h, packed.ctypes.data, None if af is None else af.ctypes.data,
                                                   status.ctypes.data))
        bad = np.flatnonzero(status)
        if len(bad):
            k = int(bad[0])
            raise ValueError(f"{self.store.path}: `data` chunk at row {batch[k][0]}: "
                             f"{LZF_ERRORS.get(int(status[k]), f'status {int(status[k])}')}")
        return batch[0][0], packed, af

    def __iter__(self):
        inflight = []
        with open(self.store.path, "rb") as fh:
            for batch in self._plan():
                inflight.append(self._submit(fh, batch))
                if len(inflight) == 2:
                    yield self._fetch(*inflight.pop(0))
            while inflight:
                yield self._fetch(*inflight.pop(0))


def pack_rows(cells):
    """Host form of k_h5_pack: (packbits rows, AF float32 or None); raises ValueError on a mixed float32 row."""
    packed = np.packbits(cells != 0, axis=1)
    if cells.dtype != np.float32:
        return packed, None
    nz = cells != 0
    has = nz.any(axis=1)
    common = np.where(has, cells[np.arange(len(cells)), nz.argmax(axis=1)], np.float32(0)).astype(np.float32)
    bad = (nz & (cells != common[:, None])).any(axis=1) | (nz & ~(cells > 0)).any(axis=1)
    if bad.any():
        raise ValueError(f"row {int(np.flatnonzero(bad)[0])}: {LZF_ERRORS[5]}")
    return packed, common
