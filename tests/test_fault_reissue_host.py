"""Host: the fault re-issue helpers of runtime.py (per_step_kernels, fault_bits, reissue_per_step) against a scripted
`take_fault`, with a dummy owner of the `persistent` switch and a dummy `fallbacks` counter.  No GPU."""
import types

import pytest
import torch

from speaker_follower_amd import runtime

CUDA = torch.device('cuda', 0)          # (a device OBJECT: nothing here touches a GPU)


@pytest.fixture
def scripted(monkeypatch):
    """runtime.take_fault replaced by a function that hands out `script` front to back and records its calls."""
    script, calls = [], []

    def take_fault(device):
        calls.append(device)
        return script.pop(0)
    monkeypatch.setattr(runtime, 'take_fault', take_fault)
    return script, calls


def things(persistent=True):
    return types.SimpleNamespace(persistent=persistent), types.SimpleNamespace(fallbacks=0)


def test_the_switch_is_off_inside_and_back_afterwards():
    for before in (True, False):
        owner, _ = things(before)
        with runtime.per_step_kernels(owner):
            assert owner.persistent is False
        assert owner.persistent is before
    with runtime.per_step_kernels(None):                # (nothing to switch)
        pass
    bare = types.SimpleNamespace()                      # (an owner that never set the switch: on by default)
    with runtime.per_step_kernels(bare):
        assert bare.persistent is False
    assert bare.persistent is True


def test_the_switch_is_restored_when_the_body_raises(scripted):
    script, calls = scripted
    owner, counter = things()

    def body():
        assert owner.persistent is False
        raise KeyError('inside')
    with pytest.raises(KeyError):
        runtime.reissue_per_step(owner, counter, CUDA, 'a pass', body, bits=2)
    assert owner.persistent is True and counter.fallbacks == 1 and calls == []


def test_one_reissue_counts_once_and_returns_what_the_body_returned(scripted):
    script, calls = scripted
    owner, counter = things()
    seen = []

    def body():
        seen.append(owner.persistent)
        return 'state %d' % len(seen)
    for n in (1, 2, 3):
        script.append(0)
        assert runtime.reissue_per_step(owner, counter, CUDA, 'a pass', body, bits=1) == 'state %d' % n
        assert counter.fallbacks == n and owner.persistent is True
    assert seen == [False] * 3 and calls == [CUDA] * 3           # (one read of the fault words per re-issue, behind the body)


def test_a_second_fault_raises_and_names_both_bit_sets_and_the_pass(scripted):
    script, calls = scripted
    owner, counter = things()
    script.append(4)
    with pytest.raises(runtime.PersistentLaunchFault) as e:
        runtime.reissue_per_step(owner, counter, CUDA, 'a route scoring pass', lambda: None, bits=3)
    assert str(e.value) == 'fault bits 3, and 4 after the per-step re-issue of a route scoring pass'
    assert owner.persistent is True and counter.fallbacks == 1   # (restored when the check raises; counted before)


def test_no_owner_and_no_counter_are_accepted(scripted):
    script, calls = scripted
    script.append(0)
    assert runtime.reissue_per_step(None, None, CUDA, 'a pass', lambda: 7) == 7
    _, counter = things()
    script.append(0)
    assert runtime.reissue_per_step(None, counter, CUDA, 'a pass', lambda: 8) == 8 and counter.fallbacks == 1


def test_fault_bits_of_a_cpu_device_are_zero_without_a_read(scripted):
    script, calls = scripted
    assert runtime.fault_bits(torch.device('cpu')) == 0 and calls == []
    script.append(5)
    assert runtime.fault_bits(CUDA) == 5 and calls == [CUDA]
    # (a re-issue on a CPU device -- the speaker's eager loop with modules on the host -- reads nothing either)
    assert runtime.reissue_per_step(None, None, torch.device('cpu'), 'a pass', lambda: 1) == 1 and calls == [CUDA]
