#!/usr/bin/env python3
"""Writes decode_group_chain.json: what the library named by LSMGPU_LIB (default: the built
one) gives for the status batch of tests/test_gpu_decode_group_chain.py, with and without
LSM_DECODE_PAYLOAD_VERIFIED, through lsm_decode_blocks and lsm_decode_blocks16.  Needs a GPU.
The committed file was written from the build of the commit before the group kernel's
header step moved to the phase-A wave.

usage: tests/golden/make_decode_group_chain.py [OUT.json]
"""
import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent.parent
for p in (ROOT, ROOT / "oracle", ROOT / "lsm-tree_amd", ROOT / "tests"):
    sys.path.insert(0, str(p))

import lsmgpu  # noqa: E402
import test_gpu_decode_group_chain as T  # noqa: E402


def main():
    out = {"batch": {str(b): what for b, (what, _) in T.STATUS_FAULTS.items()}}
    buf, off = T.status_batch()
    _, item_start, _ = T.oracle_of("status", 0)
    starts = item_start.astype("int64")
    for name, flags in (("plain", 0), ("verified", T.PAYLOAD_VERIFIED)):
        out[name] = {}
        for compact in (False, True):
            runs = []
            for given in (None, item_start):
                g = T.decode_canary(lsmgpu, buf, off, compact, given, expect_type=0, flags=flags)
                runs.append(([int(x) for x in g["status"]], T.digests(g, g["status"], starts, compact)))
            assert runs[0] == runs[1], "item_start given or not must not matter"
            out[name]["blocks16" if compact else "blocks"] = {"status": runs[0][0], "sha256": runs[0][1]}
    dst = Path(sys.argv[1]) if len(sys.argv) > 1 else HERE / "decode_group_chain.json"
    dst.parent.mkdir(parents=True, exist_ok=True)
    dst.write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps({k: v["blocks"]["status"] for k, v in out.items() if k != "batch"}))


if __name__ == "__main__":
    main()
