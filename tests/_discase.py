"""TEST INFRASTRUCTURE: the scenes the DIS dense optical flow is tested on (statement, host-interpreted kernels, device alike): those of tests/_flowcase.py, imported
and not edited, with the statement's result (tests/_disstmt.flow_dis) of each scene at each finest scale computed once, shared and never modified.

  cut-200x168 (stride 208)  scales 3, 2 at the reference's finest scale 2 (3, 2, 1 at 1): level 3 is 25 x 21 — a halved odd side, and a last row no patch covers
  odd-384x216               scales 4, 3, 2: level 4 is 24 x 13 — an uncovered row, two patch rows
  exits-96x64               coarsest = 2, at the reference's finest scale a single level of 24 x 16: ramps displaced by +-40 and 12 px take the clamped sampling through every side and
                            the return-to-start rule
256 x 24 is the size that is refused: coarsest = min(3, 1) = 1 is under the reference's finest scale 2."""
import numpy as np

import _disstmt as DS
import _flowcase as FC

SPECS, EXIT_SPECS, ALL_SPECS = FC.SPECS, FC.EXIT_SPECS, FC.ALL_SPECS
FINEST = (2, 1)
REFUSED_SIZE = (256, 24)
LEVELS = {(200, 168): [(200, 168), (100, 84), (50, 42), (25, 21)], (384, 216): [(384, 216), (192, 108), (96, 54), (48, 27), (24, 13)],
          (96, 64): [(96, 64), (48, 32), (24, 16)], (256, 24): [(256, 24), (128, 12)]}
OUTPUTS = ("grid_points", "grid_counts", "pair_first", "points_a", "points_b", "flow")
_STMT = {}


def case(name):
    return FC.case(name)


CONFIGS = [(name, f) for name in sorted(ALL_SPECS) for f in FINEST]


def statement(name, finest):
    """-> (the statement's outputs, the traces of its pairs)"""
    if (name, finest) not in _STMT:
        c = case(name)
        traces = []
        s = DS.flow_dis(c.frames[:, :, :c.width], c.pairs, finest, traces)
        for a in s.values():
            a.setflags(write=False)
        _STMT[(name, finest)] = (s, traces)
    return _STMT[(name, finest)]


def assert_equal_to_statement(got, want, what, names=OUTPUTS):
    FC.assert_equal_to_statement(got, want, what, names)
