#!/usr/bin/env python3
"""Record tests/golden/place_eval_digests.json (needs the GPU).

Drives every scenario of tests/test_gpu_place_eval.py through the legacy
batch driver, timing on and off, and writes the digests that its
test_matches_parent_digests compares both drivers with. The fixture pins
the placer kernels to what a given commit computed, so record it in a
checkout of that commit's csrc/ and gpu_placer.py (with this tool and the
test file copied in), never from the code under test:

    python tools/record_place_eval_digests.py --commit <sha> [--out FILE]
        [--left-out KEY ...]

Record twice, in two processes, and compare the files. A key on which
two recordings of the same commit disagree is named with --left-out and
stays out of the fixture. Same protocol as tools/record_place_digests.py.
"""
import argparse
import importlib.util
import json
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
TEST = ROOT / "tests" / "test_gpu_place_eval.py"


def _line(cmd):
    try:
        out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True,
                             check=True).stdout
    except (OSError, subprocess.CalledProcessError):
        return "unknown"
    return next((ln.strip() for ln in out.splitlines() if ln.strip()),
                "unknown")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--commit", default=None,
                    help="commit the kernels come from (default: HEAD)")
    ap.add_argument("--out", type=Path, default=None)
    ap.add_argument("--left-out", nargs="*", default=[])
    args = ap.parse_args()

    sys.path.insert(0, str(ROOT))
    spec = importlib.util.spec_from_file_location("test_gpu_place_eval", TEST)
    t = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(t)

    digests = {}
    for name in t.CASES:
        for timing in (False, True):
            d = t._digests(t._drive(name, timing, True))
            for snap in d.values():
                for k in args.left_out:
                    del snap[k]
            digests[f"{name}-{'timing' if timing else 'bb'}"] = d
    doc = {
        "recorded_from": args.commit or _line(["git", "rev-parse", "HEAD"]),
        "hipcc": _line(["hipcc", "--version"]),
        "driver": "legacy (pnr_place_batch)",
        "left_out": sorted(args.left_out),
        "digests": digests,
    }
    out = args.out or t.DIGESTS
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(doc, indent=1) + "\n")
    print(f"wrote {out}: {len(digests)} scenarios")


if __name__ == "__main__":
    main()
