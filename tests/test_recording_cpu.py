"""CPU checks of hip.recording, the only code that sets hip.RECORDER (capture.build records command lists through it).
cris_bn_partials_rows(0) returns 0 without touching a device, so it can be recorded and replayed here."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hip():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.build()
    from cris.pytorch_amd import hip
    return hip


def test_recording_records_calls_and_resets(hip):
    cl = hip.CommandList()
    with hip.recording(cl) as rec:
        assert rec is cl and hip.RECORDER is cl
        hip.call("cris_bn_partials_rows", 0)
    assert hip.RECORDER is None
    assert [name for _, _, name in cl.cmds] == ["cris_bn_partials_rows"]
    cl.replay()
    hip.call("cris_bn_partials_rows", 0)                 # not recording any more
    assert len(cl.cmds) == 1


def test_recording_refuses_to_nest(hip):
    outer, inner = hip.CommandList(), hip.CommandList()
    with hip.recording(outer):
        with pytest.raises(RuntimeError, match="already being recorded"):
            with hip.recording(inner):
                pass
        assert hip.RECORDER is outer
    assert hip.RECORDER is None


def test_recording_resets_after_an_exception(hip):
    cl = hip.CommandList()
    with pytest.raises(ValueError):
        with hip.recording(cl):
            hip.call("cris_bn_partials_rows", 0)
            raise ValueError("body failed")
    assert hip.RECORDER is None
    with hip.recording(cl):                              # usable again
        pass
    assert hip.RECORDER is None
