"""Hand-made malformed BCF files for the BCF reader's tests (CPU restatement, CPU build of the device code, GPU reader):
a small good stream of 8 records x 2 samples from bcf_gen, with record BAD (counted from 0) rewritten per case."""
import struct

import bcf_gen

HEAD = "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tA\tB\n"
GOOD = "c\t1\t.\tA\tC\t.\t.\t.\tGT\t0|1\t1|1\n"
LAST = "c\t2\t.\tA\tC,G\t.\t.\t.\tGT\t0|2\t2|2\n"
N_REC, BAD = 8, 3

# case -> what the error must say (the reason, word for word as bcfio and the library give it)
RECORD_CASES = {
    "truncated-file": "truncated record",
    "short-l-shared": "l_shared below 24",
    "field-past-l-indiv": "a FORMAT field that runs past l_indiv",
    "float-gt": "a GT field that is not of an integer type",
    "wrong-n-sample": "n_sample differs from the header's sample count",
    "no-gt": "no GT among the FORMAT fields",
}
FILE_CASES = {"bad-magic": "magic", "bad-magic-in-bgzf": "bad magic", "corrupted-member": "member"}


def good_vcf():
    return (HEAD + GOOD * (N_REC - 1) + LAST).encode()


def _with_indiv(rec, indiv):
    l_shared = struct.unpack_from("<I", rec, 0)[0]
    return struct.pack("<II", l_shared, len(indiv)) + rec[8:8 + l_shared] + indiv


def bad_stream(case, bad=BAD):
    """Record `bad` (counted from 0) rewritten -> (raw stream bytes, number of the record the error names, counted from 1)."""
    head, recs = bcf_gen.split_stream(bcf_gen.make_bcf(good_vcf(), raw=True))
    rec = recs[bad]
    l_shared = struct.unpack_from("<I", rec, 0)[0]
    indiv = rec[8 + l_shared:]            # key (0x11, index), descriptor 0x21 (int8 x 2), 2 samples x 2 bytes
    assert len(indiv) == 7 and indiv[0] == 0x11 and indiv[2] == 0x21
    named = bad + 1
    if case == "truncated-file":
        return head + b"".join(recs)[:-5], N_REC
    if case == "short-l-shared":
        rec = struct.pack("<I", 10) + rec[4:]
    elif case == "field-past-l-indiv":
        rec = rec[:8 + l_shared + 2] + b"\x41" + rec[8 + l_shared + 3:]      # int8 x 4: 8 bytes where 4 are left
    elif case == "float-gt":
        rec = _with_indiv(rec, indiv[:2] + b"\x15" + struct.pack("<ff", 1.0, 2.0))
    elif case == "wrong-n-sample":
        rec = rec[:28] + struct.pack("<I", 1 << 24 | 3) + rec[32:]
    elif case == "no-gt":
        rec = rec[:8 + l_shared + 1] + b"\x63" + rec[8 + l_shared + 2:]      # another key
    else:
        raise KeyError(case)
    return head + b"".join(recs[:bad] + [rec] + recs[bad + 1:]), named


def bad_file(case):
    """File-level damage -> file bytes."""
    from utmos_amd.vcfgpu import bgzf_compress, bgzf_members
    stream = bcf_gen.make_bcf(good_vcf(), raw=True)
    if case == "bad-magic":
        return b"BCX" + stream[3:]
    if case == "bad-magic-in-bgzf":
        return bgzf_compress(b"BCF\x03" + stream[4:], block=300)
    if case == "corrupted-member":
        data = bytearray(bgzf_compress(stream, block=300))
        off, size, _ = bgzf_members(bytes(data))[-2]          # the last member that holds text
        data[off + size - 12] ^= 0x5A                         # inside its deflate data
        return bytes(data)
    raise KeyError(case)
