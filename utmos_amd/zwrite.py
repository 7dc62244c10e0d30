"""zlib streams compressed on the GPU (csrc/deflate.hip.h, utm_deflate_*): a file-like writer for joblib part files.

`GpuZlibWriter` takes bytes through `write`, fills the context's pinned staging, and pushes every full batch while the
caller goes on writing; the compressed bytes of earlier batches are written to the file as they come back.  The file is
one standard zlib stream (RFC 1950: header, raw DEFLATE of independent 64 KiB segments, Adler-32), which `zlib`,
`joblib.load` and every inflater read.
"""
import ctypes

from . import _native as nat

DEFAULT_BATCH = 32 << 20


def zlib_header(level):
    """The two zlib header bytes zlib itself writes for `level` (32 KiB window, FLEVEL from the level)."""
    flevel = 0 if level < 2 else 1 if level < 6 else 2 if level == 6 else 3
    cmf = 0x78
    flg = flevel << 6
    flg |= 31 - ((cmf << 8) | flg) % 31
    return bytes([cmf, flg])


class GpuZlibWriter:
    """A write-only binary file object whose bytes land in `path_or_file` as one zlib stream compressed on `device`.

    `tell()` is the count of uncompressed bytes written, as for gzip / zlib file objects.  `close()` compresses the
    tail and writes the Adler-32 trailer (and keeps the context's `timing()` in `final_timing`); it closes the file
    only when the writer opened it."""

    def __init__(self, path_or_file, level=5, device=0, batch_bytes=DEFAULT_BATCH):
        if not 1 <= int(level) <= 9:
            raise ValueError(f"level {level} not in [1, 9]")
        self._lib = nat.lib()
        h = ctypes.c_void_p()
        nat.check(self._lib.utm_deflate_create(int(device), int(batch_bytes), int(level), ctypes.byref(h)))
        self._h = h
        buf, cap = ctypes.c_void_p(), ctypes.c_uint64()
        nat.check(self._lib.utm_deflate_staging(h, ctypes.byref(buf), ctypes.byref(cap)))
        self._stage = (ctypes.c_char * cap.value).from_address(buf.value)
        self._view = memoryview(self._stage).cast("B")
        self._cap = cap.value
        self._fill = 0
        self._pos = 0
        self._pending = 0
        self._own = isinstance(path_or_file, (str, bytes)) or hasattr(path_or_file, "__fspath__")
        self._fh = open(path_or_file, "wb") if self._own else path_or_file
        self._fh.write(zlib_header(int(level)))
        self.closed = False

    # -- file protocol
    def writable(self):
        return True

    def tell(self):
        return self._pos

    def write(self, data):
        if self.closed:
            raise ValueError("write to a closed GpuZlibWriter")
        src = memoryview(data).cast("B")
        n, off = len(src), 0
        while off < n:
            k = min(n - off, self._cap - self._fill)
            self._view[self._fill:self._fill + k] = src[off:off + k]
            self._fill += k
            off += k
            if self._fill == self._cap:
                self._push(0)
        self._pos += n
        return n

    def flush(self):
        pass

    def close(self):
        if self.closed:
            return
        try:
            self._push(1)
            while self._pending:
                self._pull()
            adler = ctypes.c_uint32()
            nat.check(self._lib.utm_deflate_adler(self._h, ctypes.byref(adler)))
            self._fh.write(adler.value.to_bytes(4, "big"))
            self.final_timing = self.timing()
        finally:
            self._release()

    def timing(self):
        """HIP-event ms so far: {"h2d", "kernels", "d2h", "parse"} (parse is part of kernels)."""
        ms = (ctypes.c_double * 4)()
        nat.check(self._lib.utm_deflate_timing(self._h, ms))
        return dict(zip(("h2d", "kernels", "d2h", "parse"), ms))

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            self.close()
        else:
            self._release()
        return False

    def __del__(self):
        if not getattr(self, "closed", True):
            self._release()

    # -- batches
    def _push(self, flags):
        if self._pending == 2:
            self._pull()
        nat.check(self._lib.utm_deflate_push(self._h, ctypes.addressof(self._stage), self._fill, flags))
        self._pending += 1
        self._fill = 0

    def _pull(self):
        ptr, n = ctypes.c_void_p(), ctypes.c_uint64()
        self._pending -= 1
        nat.check(self._lib.utm_deflate_pull(self._h, ctypes.byref(ptr), ctypes.byref(n)))
        if n.value:
            self._fh.write((ctypes.c_char * n.value).from_address(ptr.value))

    def _release(self):
        self.closed = True
        self._view.release()
        self._stage = None
        if self._h:
            self._lib.utm_deflate_destroy(self._h)
            self._h = None
        if self._own:
            self._fh.close()


def zlib_compress(data, level=5, device=0, batch_bytes=DEFAULT_BATCH):
    """bytes -> one zlib stream compressed on the GPU (what `zlib.decompress` reads back)."""
    import io
    out = io.BytesIO()
    with GpuZlibWriter(out, level, device, batch_bytes) as w:
        w.write(data)
    return out.getvalue()


def deflate_host(data, level=5):
    """-> (raw deflate bytes, Adler-32) from the CPU build of the device encoder (utm_deflate_host); needs no GPU."""
    lib = nat.lib()
    data = bytes(data)
    bound = ctypes.c_uint64()
    nat.check(lib.utm_deflate_bound(len(data), ctypes.byref(bound)))
    out = ctypes.create_string_buffer(bound.value)
    n, adler = ctypes.c_uint64(), ctypes.c_uint32()
    nat.check(lib.utm_deflate_host(data, len(data), int(level), out, bound.value, ctypes.byref(n), ctypes.byref(adler)))
    return out.raw[:n.value], adler.value
