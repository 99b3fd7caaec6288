"""A strict parser of the LZ4 block format, for the streams lsm_lz4_compress_blocks
writes.  lz4_check(stream, raw_len) decodes the stream and raises Lz4FormatError on
any breach of the rules a conforming compressor keeps (lz4 block format
specification, "End of block restrictions"), which liblz4's decoder relies on and
lz4_flex's does not check:

  * every offset is in 1..65535 and <= the bytes already produced;
  * every match is >= 4 bytes (the format cannot say less);
  * the last sequence is literals only, and ends exactly at the stream's end;
  * the last 5 bytes of the output are literals;
  * no match starts within the last 12 bytes of the output;
  * so an output shorter than 13 bytes is all literals;
  * the decoded length is raw_len.

Two layers: parse_sequences turns the bytes into (literals, offset, match_len)
sequences (offset None: the last, literals-only sequence), check_sequences applies
the rules to such a list.  The 2-byte offset field cannot hold 65536, so that rule
is only reachable through check_sequences.
"""


class Lz4FormatError(ValueError):
    pass


def _length(stream, ip, nibble):
    n = nibble
    if nibble == 15:
        while True:
            if ip >= len(stream):
                raise Lz4FormatError("truncated length extension")
            b = stream[ip]
            ip += 1
            n += b
            if b != 255:
                break
    return n, ip


def parse_sequences(stream):
    stream = bytes(stream)
    if not stream:
        raise Lz4FormatError("empty stream (an empty block is the one byte 00)")
    seqs = []
    ip = 0
    while True:
        if ip >= len(stream):
            raise Lz4FormatError("the stream ends after a match: the last sequence is not literals only")
        token = stream[ip]
        ip += 1
        lit, ip = _length(stream, ip, token >> 4)
        if lit > len(stream) - ip:
            raise Lz4FormatError("truncated literals")
        literals = stream[ip:ip + lit]
        ip += lit
        if ip == len(stream):
            if token & 15:
                raise Lz4FormatError("the last sequence carries a match length")
            seqs.append((literals, None, 0))
            return seqs
        if len(stream) - ip < 2:
            raise Lz4FormatError("truncated offset")
        off = stream[ip] | (stream[ip + 1] << 8)
        ip += 2
        ml, ip = _length(stream, ip, token & 15)
        seqs.append((literals, off, ml + 4))


def check_sequences(seqs, raw_len):
    out = bytearray()
    matches = []  # (start, end) in the output
    if not seqs or seqs[-1][1] is not None:
        raise Lz4FormatError("the last sequence is not literals only")
    for literals, off, ml in seqs[:-1]:
        out += literals
        if off is None:
            raise Lz4FormatError("a literals-only sequence before the last one")
        if off == 0:
            raise Lz4FormatError("offset 0")
        if off > 65535:
            raise Lz4FormatError(f"offset {off} above 65535")
        if off > len(out):
            raise Lz4FormatError(f"offset {off} beyond the {len(out)} bytes produced")
        if ml < 4:
            raise Lz4FormatError(f"match of {ml} bytes")
        start = len(out)
        if off >= ml:
            out += out[start - off:start - off + ml]
        else:
            pattern = bytes(out[start - off:])
            out += (pattern * (ml // off + 1))[:ml]
        matches.append((start, start + ml))
    out += seqs[-1][0]
    if len(out) != raw_len:
        raise Lz4FormatError(f"decoded {len(out)} bytes, expected {raw_len}")
    for start, end in matches:
        if end > raw_len - 5:
            raise Lz4FormatError(f"match [{start}, {end}) reaches into the last 5 bytes of {raw_len}")
        if start > raw_len - 12:
            raise Lz4FormatError(f"match starts at {start}, within the last 12 bytes of {raw_len}")
    if raw_len < 13 and matches:
        raise Lz4FormatError("an output shorter than 13 bytes must be all literals")
    return bytes(out)


def lz4_check(stream, raw_len):
    return check_sequences(parse_sequences(stream), raw_len)
