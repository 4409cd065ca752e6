#!/usr/bin/env python3
"""Host-clock time of a context's whole life:   python tools/context_cycles.py [--cycles 50] [--width 1920 --height 1080]

Cycles of rt_create -> rt_resize -> rt_destroy on device 0, after two cycles that are not timed, through the library that
RT_AMD_LIB names (default: this tree's).  Prints one line (results of its first use: profiles/refactor_owners.txt)."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import raytracing_engine_amd as R  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cycles", type=int, default=50)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    args = ap.parse_args()
    ms = []
    for k in range(args.cycles + 2):
        t0 = time.perf_counter()
        r = R.Renderer(0)
        r.resize(args.width, args.height)
        r.close()
        if k >= 2:
            ms.append((time.perf_counter() - t0) * 1e3)
    print(f"{args.cycles} cycles of rt_create -> rt_resize({args.width}, {args.height}) -> rt_destroy: total {sum(ms):.1f} ms, "
          f"median {statistics.median(ms):.3f} ms, min {min(ms):.3f} ms, max {max(ms):.3f} ms  ({os.environ.get('RT_AMD_LIB', 'this tree')})")


if __name__ == "__main__":
    main()
