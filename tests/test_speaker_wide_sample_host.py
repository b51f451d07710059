"""CPU: the host side of `sample` feedback over vocabularies of more than 1 024 words (wide_sample): the new C-ABI
symbol, the vocabulary check the engines make before anything is launched, and the defaults of the switches."""
import pytest


def test_sample_max_vocab_symbol_and_abi_version():
    import ctypes
    from speaker_follower_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, 'sf_speaker_sample_max_vocab')
    assert 'sf_speaker_sample_max_vocab' in _lib.EXPORTS
    assert _lib.lib.sf_speaker_sample_max_vocab() == 4096
    assert _lib.ABI_VERSION == 10 and _lib.lib.sf_abi_version() == 10     # (additive; 10 is the removal of the retired schedules' fields)


def test_check_sample_vocab():
    from speaker_follower_amd import speaker
    assert speaker.check_sample_vocab(1024, False) is None
    assert speaker.check_sample_vocab(991, True) is None
    with pytest.raises(NotImplementedError, match='wide_sample') as e:
        speaker.check_sample_vocab(1025, False)
    assert '4096' in str(e.value) and '1025' in str(e.value)              # names the switch and the limit
    assert speaker.check_sample_vocab(1025, True) is None
    assert speaker.check_sample_vocab(4096, True) is None
    with pytest.raises(NotImplementedError, match='4096'):
        speaker.check_sample_vocab(4097, True)
    with pytest.raises(NotImplementedError, match='4096'):
        speaker.check_sample_vocab(4097, False)


def test_the_switches_are_off_by_default():
    import inspect
    from speaker_follower_amd import agents, speaker
    assert speaker.SpeakerEngine.wide_sample is False
    assert agents.Seq2SeqSpeaker.wide_sample is False
    assert inspect.signature(speaker.SpeakerSweep.__init__).parameters['wide_sample'].default is False
