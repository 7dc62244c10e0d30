"""Test helper: a plain Python restatement of the LZF compressor h5py's filter runs (liblzf's lzf_compress, ULTRA_FAST
index, HLOG = 17, a fresh zeroed table per chunk, the `ip + 4 < in_end` match rule), output capacity included.
It is the specification utm_lzf_encode_host and the device encoder are held to (tests/test_h5w_host.py)."""

HLOG = 17
HSIZE = 1 << HLOG
MAX_LIT = 32
MAX_OFF = 1 << 13
MAX_REF = (1 << 8) + (1 << 3)


def _idx(h):
    return ((h >> (24 - HLOG)) - h) & (HSIZE - 1)


def lzf_compress(data, out_len=None):
    """bytes -> compressed bytes, or None when they do not fit in `out_len` bytes (default: len(data), as h5py's
    filter gives it; the chunk is then stored raw)."""
    ip = bytes(data)
    n = len(ip)
    out_len = n if out_len is None else out_len
    if n == 0 or out_len == 0:
        return None
    htab = [0] * HSIZE
    out = bytearray(out_len + 4)
    op, lit, p = 1, 0, 0
    h = (ip[0] << 8 | ip[1]) if n >= 2 else 0
    while p < n - 2:
        h = ((h << 8) | ip[p + 2]) & 0xFFFFFFFF
        slot = _idx(h)
        r = htab[slot]
        htab[slot] = p
        if r > 0 and p - r - 1 < MAX_OFF and p + 4 < n and ip[r:r + 3] == ip[p:p + 3]:
            off = p - r - 1
            maxlen = min(MAX_REF, n - p - 2)
            length = 2
            while True:
                length += 1
                if not (length < maxlen and ip[r + length] == ip[p + length]):
                    break
            if op + 4 >= out_len and op - (lit == 0) + 4 >= out_len:
                return None
            out[op - lit - 1] = (lit - 1) & 0xFF
            op -= lit == 0
            code = length - 2
            if code < 7:
                out[op] = (off >> 8) + (code << 5)
                op += 1
            else:
                out[op] = (off >> 8) + (7 << 5)
                out[op + 1] = code - 7
                op += 2
            out[op] = off & 0xFF
            op += 2                               # the byte and a new run's control byte
            lit = 0
            p += length
            if p >= n - 2:
                break
            q = p - 1
            h = (ip[q] << 8 | ip[q + 1])
            h = ((h << 8) | ip[q + 2]) & 0xFFFFFFFF
            htab[_idx(h)] = q
        else:
            if op >= out_len:
                return None
            out[op] = ip[p]
            op += 1
            p += 1
            lit += 1
            if lit == MAX_LIT:
                out[op - lit - 1] = lit - 1
                lit = 0
                op += 1
    if op + 3 > out_len:
        return None
    while p < n:
        out[op] = ip[p]
        op += 1
        p += 1
        lit += 1
        if lit == MAX_LIT:
            out[op - lit - 1] = lit - 1
            lit = 0
            op += 1
    out[op - lit - 1] = (lit - 1) & 0xFF
    op -= lit == 0
    return bytes(out[:op])
