"""The payloads the LZ4 compression tests share (tests/test_lz4_compress_cpu.py,
tests/test_gpu_lz4_compress.py): encoded data blocks of the usual item shapes,
JSON-valued rows that compress about 3x, and the edge lengths of the block format.
corpus() -> list of (name, payload bytes), built once per process."""
import functools

import numpy as np

import pyoracle
from helpers import counter_items, prefix_items, random_sorted_items

EDGE_LENGTHS = (0, 1, 4, 5, 11, 12, 13, 14, 63, 64, 65, 4096, 65535, 65536)


def json_rows(n):
    """(key, value, seqno, value type) rows with JSON-like values: about 3x under liblz4."""
    return [(b"user%08d" % (3 * i),
             b'{"user":%d,"name":"user%05d","active":true,"score":%d}' % (i, i, (i * 7919) % 1000), 63, 0)
            for i in range(n)]


def json_items(n):
    return pyoracle.Items.from_list(json_rows(n))


def json_block(n, restart_interval=16):
    return pyoracle.data_block_encode(json_items(n), restart_interval=restart_interval)


def pattern_payload(n, pattern=b"abcdefg"):
    return (pattern * (n // len(pattern) + 1))[:n]


@functools.lru_cache(maxsize=None)
def corpus():
    out = []
    for n in (52, 205, 820):
        out.append((f"counter{n}", pyoracle.data_block_encode(counter_items(n), restart_interval=16)))
    for n in (52, 820):
        out.append((f"random_sorted{n}", pyoracle.data_block_encode(random_sorted_items(n), restart_interval=16)))
    out.append(("prefix56", pyoracle.data_block_encode(prefix_items(56), restart_interval=16)))
    for n in (52, 205, 820, 1300):
        out.append((f"json{n}", json_block(n)))
    out.append(("random5000", np.random.default_rng(11).integers(0, 256, 5000, dtype=np.uint8).tobytes()))
    out.append(("zeros9000", bytes(9000)))
    out.append(("fox", b"the quick brown fox jumps over the lazy dog " * 200))
    for n in EDGE_LENGTHS:
        out.append((f"pattern{n}", pattern_payload(n)))
    return out


def frame(payload, block_type=0):
    """Header || payload as lsm_encode_blocks writes it (CompressionType::None)."""
    return pyoracle.block_header(block_type, payload, len(payload)) + payload
