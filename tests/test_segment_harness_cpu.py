"""The refusal loop of tests/_segment_harness.py can still fail: a call that touches one element of one output is caught."""
import numpy as np
import pytest

from _segment_harness import OUT_FILL, STACK_FILL, refusals


def test_a_touched_output_is_caught():
    seen = []

    def fake(expect, touch=None, outs="pns", **kw):
        seen.append((expect, kw))
        got = [np.full((2, 3), OUT_FILL, np.float32) if "p" in outs else None, np.full(4, OUT_FILL, np.int32) if "n" in outs else None,
               np.full((2, 2), STACK_FILL) if "s" in outs else None]
        if touch is not None:
            got[touch].flat[1] += 1
        return tuple(got)

    refused = refusals(fake, prm="valid", flags=0x80)
    refused(-2, prm="bad")                                    # untouched outputs pass, and the call saw the bad keyword over the valid
    refused(-1, outs="")
    assert seen[0] == (-2, {"prm": "bad", "flags": 0x80}) and seen[1][0] == -1
    for touch in (0, 1, 2):
        with pytest.raises(AssertionError):
            refused(-2, touch=touch)
