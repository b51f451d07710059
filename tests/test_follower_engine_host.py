"""Host: switches of FollowerEngine that no longer select anything."""
import pytest


def test_two_stream_forward_reads_false_and_refuses_true():
    """The two-chain forward schedule is retired.  The attribute stays because callers assign it: it
    reads False, takes False, and a true value raises instead of measuring the default schedule under another name."""
    from speaker_follower_amd import follower
    eng = follower.FollowerEngine(None, None, None)
    assert eng.two_stream_forward is False
    eng.two_stream_forward = False
    assert eng.two_stream_forward is False
    for on in (True, 1):
        with pytest.raises(ValueError, match=r'DESIGN\.md section 9'):
            eng.two_stream_forward = on
        assert eng.two_stream_forward is False
