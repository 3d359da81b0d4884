#!/usr/bin/env python3
"""How often the two pixels of a lane's pair take different matrix rows (round 8, GFW_PAIR_ROW): on frames of bench.py's C2 clip (3840x2160 YUV422P16LE, the GoPro-style
fisheye, 16 ms readout; seed 0x9F10 + j, timestamp 1000 + 33.3 j) the share of pairs (2k, 2k + 1) of a line whose rows differ, of 4-lane groups (8 pixels) and of
waves (128 pixels of one line) that hold such a pair.  The rows are the oracle's (tests/_pair_rows.py); no device needed.

usage: tools/pair_rows_count.py [frame index ...]      (default: 0 31 63)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
from gyroflow_amd import synthetic as S  # noqa: E402
import _pair_rows as P  # noqa: E402


def main():
    W, H = 3840, 2160
    print("frame  seed     pairs differing   4-lane groups   waves     max |row(x+1) - row(x)|   rows used")
    for j in [int(a) for a in sys.argv[1:]] or [0, 31, 63]:
        fr = S.SyntheticFrame("YUV422P16LE", W, H, seed=0x9F10 + j, timestamp_ms=1000.0 + 33.3 * j, lens=dict(S.gopro_style_lens(W, H)), fov=1.0,
                              interpolation=2, readout_ms=16.0, pixels=False)
        rows = P.pixel_rows(fr)
        pairs, quads, waves = P.pair_shares(rows)
        step = int(np.abs(np.diff(rows, axis=1)).max())
        print("%5d  %#06x  %14.2f %%  %12.2f %%  %6.2f %%  %10d  %20d..%d" % (j, 0x9F10 + j, 100 * pairs, 100 * quads, 100 * waves, step, rows.min(), rows.max()))


if __name__ == "__main__":
    main()
