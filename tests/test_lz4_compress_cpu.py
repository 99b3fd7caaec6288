"""CPU tests for the LZ4 compression stage (lsm_lz4_compress_blocks): the strict
block-format parser the GPU tests judge streams with (tests/lz4_check.py), the
three entry points' declaration and export, the output bound against liblz4's
sizes, and the argument checks that precede any HIP call.  No device compute."""
import ctypes as C
import re
from pathlib import Path

import pytest

from lz4_cases import handmade, lz4_compress, seq
from lz4_check import Lz4FormatError, check_sequences, lz4_check, parse_sequences
from lz4_compress_corpus import corpus

ROOT = Path(__file__).resolve().parent.parent
NEW_SYMBOLS = ("lsm_lz4_compress_bound", "lsm_lz4_compress_workspace_size", "lsm_lz4_compress_blocks")


@pytest.fixture(scope="module")
def L():
    import lsmgpu
    if not lsmgpu.LIB_PATH.exists():
        lsmgpu.build()
    return lsmgpu


@pytest.fixture(scope="module")
def liblz4_streams():
    pytest.importorskip("pyarrow")
    return [(name, p, lz4_compress(p)) for name, p in corpus()]


def test_check_accepts_liblz4_output(liblz4_streams):
    for name, p, s in liblz4_streams:
        assert lz4_check(s, len(p)) == p, name


# handmade() streams that decode and also keep the end-of-block rules (the others end
# in a match close to the end: fine for a decoder's branch coverage, not conformant)
CONFORMANT_HANDMADE = ("literals_only", "empty_block", "long_literals_ext", "unaligned_literal_runs")


def test_check_accepts_wellformed_handmade_streams():
    accepted = set()
    for name, stream, expected in handmade():
        if expected is None:
            continue
        try:
            assert lz4_check(stream, len(expected)) == expected, name
            accepted.add(name)
        except Lz4FormatError:
            pass
    assert accepted == set(CONFORMANT_HANDMADE)
    # a run and a long match that end conformantly: 6 / 12 literal bytes after the match
    assert lz4_check(seq(b"x", 1, 1000) + seq(b"THEEND"), 1007) == b"x" * 1001 + b"THEEND"
    assert lz4_check(seq(b"ab", 2, 2000) + seq(b"0123456789ab"), 2014) == b"ab" * 1001 + b"0123456789ab"


def test_check_rejects_malformed_handmade_streams():
    for name, stream, expected in handmade():
        if expected is None:
            with pytest.raises(Lz4FormatError):
                lz4_check(stream, 12)


LIT = bytes(range(32))


@pytest.mark.parametrize("name,stream,raw_len,why", [
    # 32 literals, a match of 8 at offset 8, then 4 literals: the match ends 4 bytes before the end
    ("match_into_last_5", seq(LIT, 8, 8) + seq(b"wxyz"), 44, "last 5 bytes"),
    # 32 literals, a 4-byte match starting 11 bytes before the end (7 literals follow)
    ("match_starts_in_last_12", seq(LIT, 8, 4) + seq(b"tuvwxyz"), 43, "last 12 bytes"),
    # the stream stops after a match
    ("last_sequence_has_match", seq(LIT, 8, 8), 40, "literals only"),
    ("offset_0", seq(LIT, 0, 8) + seq(b"0123456789ab"), 52, "offset 0"),
    ("offset_beyond_output", seq(LIT, 33, 8) + seq(b"0123456789ab"), 52, "beyond"),
])
def test_check_rejects_one_broken_rule(name, stream, raw_len, why):
    with pytest.raises(Lz4FormatError, match=why):
        lz4_check(stream, raw_len)


def test_check_accepts_the_same_streams_unbroken():
    """The five streams above, each with its one breach mended, pass: the rejections are
    for the named rule and nothing else."""
    assert len(lz4_check(seq(LIT, 8, 8) + seq(b"vwxyz"), 45)) == 45        # 5 literals after the match
    assert len(lz4_check(seq(LIT, 8, 4) + seq(b"stuvwxyz"), 44)) == 44     # the match starts 12 before the end
    assert len(lz4_check(seq(LIT, 32, 8) + seq(b"0123456789ab"), 52)) == 52


def test_check_rejects_offset_65536():
    """The 2-byte offset field cannot hold 65536: lz4_cases.seq refuses to build it, the
    wrapped field reads as offset 0, and the sequence-level check names the limit."""
    lit = bytes(70000)
    with pytest.raises(OverflowError):
        seq(lit, 65536, 8)
    tail = b"0123456789ab"
    assert len(check_sequences([(lit, 65535, 8), (tail, None, 0)], 70020)) == 70020
    with pytest.raises(Lz4FormatError, match="above 65535"):
        check_sequences([(lit, 65536, 8), (tail, None, 0)], 70020)
    wrapped = seq(lit, 65535, 8)[:-2] + (65536 & 0xFFFF).to_bytes(2, "little") + seq(tail)
    assert parse_sequences(wrapped)[0][1] == 0
    with pytest.raises(Lz4FormatError, match="offset 0"):
        lz4_check(wrapped, 70020)


def test_check_rejects_wrong_length():
    with pytest.raises(Lz4FormatError, match="expected"):
        lz4_check(seq(b"abc"), 4)
    with pytest.raises(Lz4FormatError):
        lz4_check(b"", 0)
    assert lz4_check(b"\x00", 0) == b""


def test_short_outputs_must_be_literals():
    # 12 output bytes with a match: every rule but the 13-byte one would pass a lax parser
    with pytest.raises(Lz4FormatError):
        lz4_check(seq(b"ab", 2, 4) + seq(b"abcdef"), 12)


def test_new_symbols_declared_exported_and_listed(L):
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "lsmgpu.h").read_text(), flags=re.S)
    declared = set(re.findall(r"\b(lsm_[a-z0-9_]+)\s*\(", text))
    lib = L.lib()
    for s in NEW_SYMBOLS:
        assert s in declared, f"{s} not declared in include/lsmgpu.h"
        assert hasattr(lib, s), f"{s} not exported"
        assert s in L.EXPORTED_SYMBOLS
    assert lib.lsm_abi_version() == 7  # additions only


def test_bound_covers_liblz4_sizes(L, liblz4_streams):
    lib = L.lib()
    total_in = sum(33 + len(p) for _, p, _ in liblz4_streams)
    total_out = sum(33 + len(s) for _, _, s in liblz4_streams)
    assert lib.lsm_lz4_compress_bound(total_in, len(liblz4_streams)) >= total_out
    sizes = {name: len(s) for name, _, s in liblz4_streams}
    assert sizes["random5000"] == 5021  # incompressible input grows
    for n in (0, 1, 12, 13, 254, 255, 256, 5000, 65535, 65536, 4 << 20):
        assert lib.lsm_lz4_compress_bound(33 + n, 1) >= 33 + n + n // 255 + 16
    for name, p, s in liblz4_streams:
        assert lib.lsm_lz4_compress_bound(33 + len(p), 1) >= 33 + len(s), name


def test_workspace_size_monotone(L):
    lib = L.lib()
    ns = (0, 1, 2, 2047, 2048, 2049, 65536, 1 << 20)
    bs = (0, 33, 4096, 1 << 20, 1 << 32)
    for b in bs:
        sizes = [lib.lsm_lz4_compress_workspace_size(n, b) for n in ns]
        assert sizes == sorted(sizes), b
    for n in ns:
        sizes = [lib.lsm_lz4_compress_workspace_size(n, b) for b in bs]
        assert sizes == sorted(sizes), n
    # room for every block's worst-case stream
    assert lib.lsm_lz4_compress_workspace_size(4, 4 * 4129) >= 4 * (4096 + 4096 // 255 + 16)


def test_bad_args_rejected_without_device(L):
    lib = L.lib()
    ws = lib.lsm_lz4_compress_workspace_size(4, 4 * 4129)
    good = [C.c_void_p(0x1000), C.c_void_p(0x2000), 4, None, C.c_void_p(0x3000), 1 << 20, C.c_void_p(0x4000),
            C.c_void_p(0x5000), C.c_void_p(0x6000), ws, None]
    # n_blocks == 0 is a no-op, whatever the pointers
    assert lib.lsm_lz4_compress_blocks(None, None, 0, None, None, 0, None, None, None, 0, None) == 0
    for i in (0, 1, 4, 6, 7, 8):  # each required buffer NULL
        a = list(good)
        a[i] = None
        assert lib.lsm_lz4_compress_blocks(*a) == 10, i
    for i, bad in ((0, 0x1008), (1, 0x2004), (3, 0x7002), (6, 0x4004), (7, 0x5002), (8, 0x6010)):  # misaligned
        a = list(good)
        a[i] = C.c_void_p(bad)
        assert lib.lsm_lz4_compress_blocks(*a) == 10, i
    a = list(good)
    a[9] = lib.lsm_lz4_compress_workspace_size(4, 0) - 1  # a short workspace
    assert lib.lsm_lz4_compress_blocks(*a) == 10

