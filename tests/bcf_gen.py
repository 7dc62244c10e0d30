"""VCF bytes -> BCF bytes in pure Python, for the BCF reader's tests: the VCFs of tests/vcf_gen.py or a fixture, written
as the format subset of DESIGN §8.4.  It shares no code with utmos_amd/bcfio.py.

The header gets ##contig, ##FILTER, ##INFO and ##FORMAT lines where the VCF has none; GT is declared last, so its
dictionary index is neither 0 nor 1.  With idx=True every line carries an IDX= that differs from the implicit numbering.
INFO values are written as strings (a long one takes the length-15 overflow), FORMAT fields other than GT as integer
vectors where every value is an integer (a long AD takes the overflow in the per-sample length), else as strings."""
import gzip
import re
import struct

INT_MISSING = {1: 0x80, 2: 0x8000, 4: 0x80000000}
WIDTH_OF = {"int8": 1, "int16": 2, "int32": 4}
TYPE_OF_WIDTH = {1: 1, 2: 2, 4: 3}
IDX_SHIFT = 5     # idx=True: dictionary index = implicit index + IDX_SHIFT (PASS stays 0)


def typed_int(v):
    """A typed integer scalar in the smallest type that holds it."""
    if -120 <= v <= 127:
        return bytes([0x11]) + struct.pack("<b", v)
    if -32760 <= v <= 32767:
        return bytes([0x12]) + struct.pack("<h", v)
    return bytes([0x13]) + struct.pack("<i", v)


def descriptor(type_code, length):
    """The descriptor byte, with the length-15 overflow (a typed integer scalar follows) from length 15 on."""
    if length < 15:
        return bytes([length << 4 | type_code])
    return bytes([0xF0 | type_code]) + typed_int(length)


def typed_string(s):
    b = s.encode()
    return descriptor(7, len(b)) + b


def int_width(lo, hi):
    if -120 <= lo and hi <= 127:
        return 1
    if -32760 <= lo and hi <= 32767:
        return 2
    return 4


def pack_ints(values, width):
    return struct.pack("<%d%s" % (len(values), {1: "B", 2: "H", 4: "I"}[width]), *[v & ((1 << 8 * width) - 1) for v in values])


def encode_gt(cells, min_width):
    """GT strings -> (width, per-sample length, bytes).  An allele is (a + 1) << 1 | phased, `.` is 0 | phased, and
    shorter calls are padded with the end-of-vector sentinel."""
    parsed = {}                      # distinct cell -> its values (call sets repeat a handful of cells)
    for cell in cells:
        if cell in parsed:
            continue
        vals = []
        for k, tok in enumerate(re.split(r"([/|])", cell)):
            if k % 2:
                phased = tok == "|"
                continue
            if k == 0:
                phased = False
            vals.append((0 if tok == "." else int(tok) + 1) << 1 | phased)
        parsed[cell] = vals
    top = max((x | 1 for v in parsed.values() for x in v), default=0)
    width = max(min_width, 1 if top <= 0x7F else 2 if top <= 0x7FFF else 4)
    length = max((len(v) for v in parsed.values()), default=0)
    eov = INT_MISSING[width] + 1
    packed = {cell: pack_ints(v + [eov] * (length - len(v)), width) for cell, v in parsed.items()}
    return width, length, b"".join(map(packed.__getitem__, cells))


def encode_field(cells):
    """A FORMAT field other than GT: an integer vector per sample when every value is an integer or `.`, else a string."""
    toks = [c.split(",") for c in cells]
    if all(re.fullmatch(r"-?\d+|\.", t) for c in toks for t in c):
        nums = [[None if t == "." else int(t) for t in c] for c in toks]
        flat = [x for c in nums for x in c if x is not None]
        width = int_width(min(flat, default=0), max(flat, default=0))
        length = max(len(c) for c in nums)
        miss, eov = INT_MISSING[width], INT_MISSING[width] + 1
        out = []
        for c in nums:
            out += [miss if x is None else x for x in c] + [eov] * (length - len(c))
        return descriptor(TYPE_OF_WIDTH[width], length) + pack_ints(out, width)
    length = max(len(c.encode()) for c in cells)
    return descriptor(7, length) + b"".join(c.encode().ljust(length, b"\0") for c in cells)


def header_and_records(vcf):
    meta, chrom, records = [], None, []
    for raw in vcf.decode().split("\n"):
        line = raw.rstrip("\r")
        if line.startswith("##"):
            if chrom is None:
                meta.append(line)
        elif line.startswith("#CHROM"):
            chrom = line
        elif line:
            records.append(line.split("\t"))
    return meta, chrom, records


def make_bcf(vcf, gt_width="auto", idx=False, raw=False, block=0xFF00, level=6, minor=2):
    """vcf: VCF bytes (plain text) -> BCF bytes.  gt_width: auto | int8 | int16 | int32 (at least that wide: a record whose
    alleles need more gets more).  raw: the bare stream, else BGZF with members of `block` bytes at `level`."""
    meta, chrom, records = header_and_records(vcf)
    declared = {kind: set(re.findall(r"##%s=<ID=([^,>]+)" % kind, "\n".join(meta))) for kind in ("contig", "FILTER", "INFO", "FORMAT")}
    contigs, filters, infos, formats = [], ["PASS"], [], []
    for f in records:
        if f[0] not in contigs:
            contigs.append(f[0])
        for x in ([] if f[6] == "." else f[6].split(";")):
            if x not in filters:
                filters.append(x)
        for kv in ([] if f[7] == "." else f[7].split(";")):
            if kv.split("=")[0] not in infos:
                infos.append(kv.split("=")[0])
        for k in f[8].split(":"):
            if k not in formats:
                formats.append(k)
    formats.sort(key=lambda k: k == "GT")      # GT last
    lines = list(meta)
    lines += ["##contig=<ID=%s>" % c for c in contigs if c not in declared["contig"]]
    lines += ['##FILTER=<ID=%s,Description="f">' % x for x in filters if x not in declared["FILTER"]]
    lines += ['##INFO=<ID=%s,Number=.,Type=String,Description="i">' % x for x in infos if x not in declared["INFO"]]
    lines += ['##FORMAT=<ID=%s,Number=.,Type=String,Description="g">' % x for x in formats if x not in declared["FORMAT"]]
    # the dictionary, numbered as the subset says (contigs have a numbering of their own)
    ids, contig_ids, out_lines = {"PASS": 0}, {}, []
    for line in lines:
        m = re.match(r"##(FILTER|INFO|FORMAT)=<ID=([^,>]+)", line)
        if m and m.group(2) not in ids:
            ids[m.group(2)] = len(ids)
        c = re.match(r"##contig=<ID=([^,>]+)", line)
        if c:
            contig_ids.setdefault(c.group(1), len(contig_ids))
    if idx:
        ids = {k: (v + IDX_SHIFT if v else 0) for k, v in ids.items()}
    for line in lines:
        m = re.match(r"##(FILTER|INFO|FORMAT)=<ID=([^,>]+)", line)
        if m and idx and "IDX=" not in line:
            line = line[:-1] + ",IDX=%d>" % ids[m.group(2)]
        out_lines.append(line)
    text = ("\n".join(out_lines + [chrom]) + "\n").encode() + b"\0"
    parts = [b"BCF\x02" + bytes([minor]) + struct.pack("<I", len(text)) + text]
    min_width = WIDTH_OF.get(gt_width, 1)
    for f in records:
        alts = [] if f[4] == "." else f[4].split(",")
        info = [] if f[7] == "." else f[7].split(";")
        keys = f[8].split(":")
        shared = struct.pack("<iii", contig_ids[f[0]], int(f[1]) - 1, len(f[3]))
        shared += struct.pack("<I", 0x7F800001) if f[5] == "." else struct.pack("<f", float(f[5]))
        shared += struct.pack("<II", (1 + len(alts)) << 16 | len(info), len(keys) << 24 | len(f) - 9)
        shared += typed_string("" if f[2] == "." else f[2])
        for a in [f[3]] + alts:
            shared += typed_string(a)
        flt = [] if f[6] == "." else [ids[x] for x in f[6].split(";")]
        shared += descriptor(1, len(flt)) + pack_ints(flt, 1)
        for kv in info:
            k, _, v = kv.partition("=")
            shared += typed_int(ids[k]) + typed_string(v)
        cells = [c.split(":") for c in f[9:]] if len(keys) > 1 else None
        indiv = b""
        for i, k in enumerate(keys):
            col = [c[i] if i < len(c) else "." for c in cells] if cells else f[9:]
            indiv += typed_int(ids[k])
            if k == "GT":
                width, length, data = encode_gt(col, min_width)
                indiv += descriptor(TYPE_OF_WIDTH[width], length) + data
            else:
                indiv += encode_field(col)
        parts.append(struct.pack("<II", len(shared), len(indiv)) + shared + indiv)
    stream = b"".join(parts)
    return stream if raw else bgzf(stream, block, level)


def bgzf(stream, block=0xFF00, level=6):
    """A raw stream in its BGZF container."""
    from utmos_amd.vcfgpu import bgzf_compress
    return bgzf_compress(stream, level=level, block=block)


def vcf_bytes(path):
    """The text of a .vcf or .vcf.gz file."""
    with (gzip.open if path.endswith(".gz") else open)(path, "rb") as fh:
        return fh.read()


def split_stream(stream):
    """A raw stream -> (magic + l_text + header text, [record bytes])."""
    l_text = struct.unpack_from("<I", stream, 5)[0]
    o, recs = 9 + l_text, []
    while o < len(stream):
        ls, li = struct.unpack_from("<II", stream, o)
        recs.append(stream[o:o + 8 + ls + li])
        o += 8 + ls + li
    return stream[:9 + l_text], recs
