"""TEST INFRASTRUCTURE: the refined statement's result (tests/_varrefstmt.flow_dis_refined) of each scene of tests/_discase.py at each finest scale and
configuration, computed once, shared by the statement, interpreter and device tests and never modified."""
import _discase as DC
import _varrefstmt as VS

DEFAULT = VS.DEFAULT
OTHER = VS.Cfg(2, 3, 12.5, 3.0, 7.0, 1.25)                  # a non-default configuration: 2 fixed-point and 3 SOR iterations, other alpha / delta / gamma / omega
_STMT = {}


def statement(name, finest, cfg=DEFAULT):
    if (name, finest, cfg) not in _STMT:
        c = DC.case(name)
        s = VS.flow_dis_refined(c.frames[:, :, :c.width], c.pairs, finest, cfg)
        for a in s.values():
            a.setflags(write=False)
        _STMT[(name, finest, cfg)] = s
    return _STMT[(name, finest, cfg)]
