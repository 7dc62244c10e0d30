"""The BGZF member decoder of csrc/inflate.hip.h, built for the CPU (utm_bgzf_inflate_host), against zlib: every block
type and zlib strategy, stored / fixed / dynamic blocks, many blocks per member, the longest and shortest distances,
empty and full-size members; and malformed members (hand-made and seeded corruption), which must come back as an error
code without reading past the member."""
import ctypes
import mmap
import zlib

import numpy as np
import pytest

import vcf_gen

# INF_E_* of inflate.hip.h
E_BTYPE, E_STORED, E_OVERSUB, E_INCOMPLETE, E_DIST, E_OUTPUT, E_INPUT, E_LENGTH, E_CRC, E_ISIZE = 2, 3, 4, 5, 8, 9, 10, 12, 13, 14
HEAD = b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00"


def inflate(member):
    """-> (code, text) from the host build of the device decoder."""
    from utmos_amd import _native as nat
    out = ctypes.create_string_buffer(65536)
    st = ctypes.c_uint32()
    nat.check(nat.lib().utm_bgzf_inflate_host(member, len(member), out, 65536, ctypes.byref(st)))
    return st.value & 255, out.raw[:min(st.value >> 8, 65536)]


def wrap(body, data, isize=None, crc=None):
    """raw deflate body -> one BGZF member of `data`."""
    crc = zlib.crc32(data) if crc is None else crc
    isize = len(data) if isize is None else isize
    return HEAD + ((len(body) + 25) & 0xFFFF).to_bytes(2, "little") + body + crc.to_bytes(4, "little") + \
        isize.to_bytes(4, "little")


def deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, pieces=1, flush=zlib.Z_FULL_FLUSH):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    step = max(1, -(-len(data) // pieces))
    body = b""
    for off in range(0, len(data), step):
        body += c.compress(data[off:off + step])
        if pieces > 1:
            body += c.flush(flush)
    return body + c.flush()


def check(data, **kw):
    code, got = inflate(wrap(deflate(data, **kw), data))
    assert code == 0 and got == data


RNG = np.random.default_rng(7)
TEXTS = {
    "empty": b"",
    "one": b"x",
    "random": RNG.integers(0, 256, 65536, dtype=np.uint8).tobytes(),       # stored blocks at every level
    "vcf": vcf_gen.make_vcf(3, 400, 60)[:65536],
    "full-vcf": (vcf_gen.make_vcf(4, 2000, 30) * 2)[:65536],
    "run": b"a" * 65536,                                                  # distance 1, length 258
    "far": RNG.integers(0, 256, 32768, dtype=np.uint8).tobytes() * 2,     # distance 32,768
    "short-period": b"ab" * 20000 + b"abc" * 5000,
}


@pytest.mark.parametrize("name", sorted(TEXTS))
@pytest.mark.parametrize("level", [0, 1, 6, 9])
def test_levels(name, level):
    check(TEXTS[name], level=level)


@pytest.mark.parametrize("name", sorted(TEXTS))
@pytest.mark.parametrize("strategy", ["Z_FIXED", "Z_RLE", "Z_HUFFMAN_ONLY", "Z_FILTERED"])
def test_strategies(name, strategy):
    check(TEXTS[name], level=6, strategy=getattr(zlib, strategy))


@pytest.mark.parametrize("flush", ["Z_FULL_FLUSH", "Z_SYNC_FLUSH"])
@pytest.mark.parametrize("pieces", [2, 17, 300])
def test_many_blocks(pieces, flush):
    data = TEXTS["vcf"]
    body = deflate(data, level=6, pieces=pieces, flush=getattr(zlib, flush))
    assert body.count(b"\x00\x00\xff\xff") >= pieces - 1     # one empty stored block per flush
    code, got = inflate(wrap(body, data))
    assert code == 0 and got == data


def test_members_of_the_bgzf_writer():
    from utmos_amd.vcfgpu import bgzf_compress, bgzf_members
    data = vcf_gen.make_vcf(5, 300, 80)
    for level in (0, 1, 6, 9):
        b = bgzf_compress(data, level=level, threads=2)
        out = b""
        for off, size, isize in bgzf_members(b):
            code, got = inflate(b[off:off + size])
            assert code == 0 and len(got) == isize
            out += got
        assert out == data


class _Bits:
    """LSB-first bit writer; Huffman codes go in most significant bit first."""

    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, value, n):
        self.v |= value << self.n
        self.n += n
        return self

    def code(self, value, n):
        return self.put(int(format(value, f"0{n}b")[::-1], 2), n)

    def bytes(self):
        return self.v.to_bytes((self.n + 7) // 8, "little")


def _fixed(*symbols):
    """A fixed-Huffman final block of literal / (length, distance) symbols."""
    b = _Bits().put(1, 1).put(1, 2)
    for s in symbols:
        if isinstance(s, int):
            b.code(0x30 + s, 8)
        else:                                  # (3, dist <= 4): length code 257, distance code dist - 1
            b.code(1, 7).code(s[1] - 1, 5)
    return b.code(0, 7).bytes()


def test_handmade_fixed_block_and_its_errors():
    assert inflate(wrap(_fixed(65, 66, (3, 2)), b"ABABA")) == (0, b"ABABA")
    assert inflate(wrap(_fixed(65, (3, 1)), b"AAAA")) == (0, b"AAAA")          # distance 1 repeats one byte
    assert inflate(wrap(_fixed((3, 1)), b"xxx"))[0] == E_DIST                  # before the start of the member
    assert inflate(wrap(_fixed(65, (3, 2)), b"AAAA"))[0] == E_DIST
    assert inflate(wrap(_fixed(65, 66, 67), b"AB"))[0] == E_OUTPUT            # more than ISIZE
    assert inflate(wrap(_fixed(65, 66), b"ABC"))[0] == E_LENGTH                # less than ISIZE
    assert inflate(wrap(_fixed(65, 66), b"AB", crc=1))[0] == E_CRC
    assert inflate(wrap(_fixed(65), b"A")[:-9] + wrap(b"", b"A")[-8:])[0] == E_INPUT   # no end-of-block


def test_handmade_block_errors():
    assert inflate(wrap(_Bits().put(1, 1).put(3, 2).bytes(), b""))[0] == E_BTYPE
    stored = _Bits().put(1, 1).put(0, 2).bytes() + (3).to_bytes(2, "little") + (0x1234).to_bytes(2, "little") + b"abc"
    assert inflate(wrap(stored, b"abc"))[0] == E_STORED
    ok = _Bits().put(1, 1).put(0, 2).bytes() + (3).to_bytes(2, "little") + (0xFFFC).to_bytes(2, "little") + b"abc"
    assert inflate(wrap(ok, b"abc")) == (0, b"abc")
    assert inflate(wrap(ok[:-1], b"abc"))[0] == E_INPUT                         # stored bytes past the member
    # dynamic headers: 19 code-length codes of length 1 (over-subscribed), one of length 2 (incomplete)
    over = _Bits().put(1, 1).put(2, 2).put(0, 5).put(0, 5).put(15, 4)
    for _ in range(19):
        over.put(1, 3)
    assert inflate(wrap(over.bytes() + b"\0" * 8, b""))[0] == E_OVERSUB
    inc = _Bits().put(1, 1).put(2, 2).put(0, 5).put(0, 5).put(0, 4).put(2, 3).put(0, 3).put(0, 3).put(0, 3)
    assert inflate(wrap(inc.bytes() + b"\0" * 8, b""))[0] == E_INCOMPLETE
    big = TEXTS["vcf"] + b"x"
    assert inflate(wrap(deflate(big), big))[0] == E_ISIZE


def test_reads_stop_at_the_member_end():
    """Members end right at a page the process may not read: any read past them faults the test."""
    libc = ctypes.CDLL(None)
    libc.mprotect.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    page = mmap.PAGESIZE
    size = 20 * page
    buf = mmap.mmap(-1, size + page)
    base = ctypes.addressof(ctypes.c_char.from_buffer(buf))
    assert libc.mprotect(base + size, page, 0) == 0
    try:
        from utmos_amd import _native as nat
        rng = np.random.default_rng(3)
        data = TEXTS["vcf"]
        good = wrap(deflate(data, 6), data)
        cases = [good, good[:40], good[:-8], wrap(_fixed(65), b"A")[:-9] + wrap(b"", b"A")[-8:]]
        for _ in range(40):
            m = bytearray(good[:int(rng.integers(18, len(good)))])
            cases.append(bytes(m))
            m = bytearray(good)
            m[int(rng.integers(18, len(m)))] ^= 1 << int(rng.integers(8))
            cases.append(bytes(m))
        out = ctypes.create_string_buffer(65536)
        st = ctypes.c_uint32()
        for m in cases:
            at = size - len(m)
            buf[at:size] = m
            nat.check(nat.lib().utm_bgzf_inflate_host(ctypes.c_void_p(base + at), len(m), out, 65536, ctypes.byref(st)))
            assert (st.value & 255) == 0 if m is good else True
    finally:
        libc.mprotect(base + size, page, 3)
        buf.close()


@pytest.mark.parametrize("seed", range(6))
def test_seeded_corruption_agrees_with_zlib(seed):
    """Bit flips in the deflate data or the trailer, truncation, ISIZE and CRC edits: the decoder accepts a member
    exactly when zlib does, with zlib's text; a member zlib rejects always comes back with an error code."""
    rng = np.random.default_rng(seed)
    data = vcf_gen.make_vcf(seed, 200, 40)[:60000]
    errors = 0
    for level, strategy in ((0, 0), (1, 0), (6, zlib.Z_FIXED), (9, zlib.Z_RLE), (6, 0)):
        good = wrap(deflate(data, level, strategy), data)
        cases = []
        for _ in range(60):
            m = bytearray(good)
            for _ in range(int(rng.integers(1, 4))):
                m[int(rng.integers(18, len(m)))] ^= 1 << int(rng.integers(8))
            cases.append(bytes(m))
        cases += [good[:int(rng.integers(18, len(good)))] for _ in range(10)]
        cases += [good[:-4] + (len(data) + d).to_bytes(4, "little") for d in (-1, 1, -len(data), 5000)]
        cases += [good[:-8] + (zlib.crc32(data) ^ (1 << int(rng.integers(32)))).to_bytes(4, "little") + good[-4:]]
        for m in cases:
            code, got = inflate(m)
            try:
                want = zlib.decompress(m, 31)
                assert len(want) == int.from_bytes(m[-4:], "little")
            except (zlib.error, AssertionError):
                want = None
            if want is None:
                assert code != 0
                errors += 1
            else:
                assert code == 0 and got == want
    assert errors > 300


def test_reader_and_command_options(tmp_path):
    import gzip
    from utmos_amd.convert import parse_args
    from utmos_amd.select import parse_args as select_args
    from utmos_amd.vcfgpu import GpuVcfReader
    with pytest.raises(ValueError, match="inflate"):
        GpuVcfReader(inflate="zlib")
    path = str(tmp_path / "one-stream.vcf.gz")
    open(path, "wb").write(gzip.compress(vcf_gen.make_vcf(1, 5, 3)))
    with pytest.raises(ValueError, match="BGZF"):          # refused before any GPU work
        GpuVcfReader(inflate="gpu").read(path)
    assert parse_args(["i.vcf.gz", "o.jl"]).inflate == "auto"
    assert parse_args(["--inflate", "host", "i.vcf.gz", "o.jl"]).inflate == "host"
    with pytest.raises(SystemExit):
        parse_args(["--inflate", "cpu", "i.vcf.gz", "o.jl"])
    assert select_args(["--inflate", "gpu", "a.jl"]).inflate == "gpu"
