"""CPU: the host side of the opt-in bf16 weight storage of the decode gate product (include/sf_hip.h:
sf_gate_product_bf16_weights): the symbols are declared, exported and bound under the unchanged ABI 9, arguments are
validated without a device, the switches read back, `gate_weights` accepts its two values only, and the caches of captured
inference graphs tell the two modes apart.  (What the kernel computes: tests/test_gpu_gate_bf16.py.)"""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ['sf_pack_bf16_bytes', 'sf_pack_bf16', 'sf_lstm_weights_bf16', 'sf_gate_product_bf16_weights',
       'sf_gate_product_bf16_weights_is_on', 'sf_gate_product_bf16_supported']


def test_symbols_are_declared_exported_and_bound_under_abi_9():
    from speaker_follower_amd import _lib
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'sf_hip.h')).read(), flags=re.S)
    raw = C.CDLL(_lib.LIB_PATH)
    for s in NEW:
        assert re.search(r'\b%s\s*\(' % s, text), '%s is not declared in sf_hip.h' % s
        assert hasattr(raw, s), 'libsf_hip.so does not export %s' % s
        assert s in _lib.EXPORTS
    assert re.search(r'#define\s+SF_ABI_VERSION\s+10\b', text)
    assert _lib.lib.sf_abi_version() == _lib.ABI_VERSION == 10
    assert C.sizeof(_lib.LstmW) == 6 * C.sizeof(C.c_void_p)               # sf_lstm_w did not grow a member


def test_packed_size_and_shape_query():
    from speaker_follower_amd._lib import lib
    assert lib.sf_pack_bf16_bytes(2048, 4352) == 2048 * 4352 * 2
    assert lib.sf_pack_bf16_bytes(80, 128) == 80 * 128 * 2
    assert lib.sf_pack_bf16_bytes(17, 64) == 32 * 64 * 2                  # rows padded to whole 16-row tiles
    for rows, K in ((0, 64), (16, 0), (16, 100), (-1, 64), (16, 32)):
        assert lib.sf_pack_bf16_bytes(rows, K) == 0
    ok = lib.sf_gate_product_bf16_supported
    assert ok(100, 4352, 512, 2048) == 1 and ok(1, 64, 0, 1) == 1 and ok(128, 128, 64, 80) == 1
    assert ok(129, 4352, 512, 2048) == 0                                  # more rows than one block holds
    assert ok(100, 4352 + 4, 512, 2048) == 0 and ok(100, 4352, 500, 2048) == 0      # K % 64
    assert ok(0, 64, 64, 64) == 0 and ok(16, 0, 64, 64) == 0 and ok(16, 64, -64, 64) == 0 and ok(16, 64, 64, 0) == 0


def test_arguments_are_validated_without_a_device():
    from speaker_follower_amd._lib import lib
    ERR_ARG = 1
    buf = C.create_string_buffer(64)
    p = C.cast(buf, C.c_void_p)
    assert lib.sf_pack_bf16(None, 64, 16, 64, p, None) == ERR_ARG
    assert lib.sf_pack_bf16(p, 64, 16, 64, None, None) == ERR_ARG
    assert lib.sf_pack_bf16(p, 64, 16, 100, p, None) == ERR_ARG            # K % 64
    assert lib.sf_pack_bf16(p, 32, 16, 64, p, None) == ERR_ARG             # ld < K
    assert lib.sf_pack_bf16(p, 66, 16, 64, p, None) == ERR_ARG             # ld % 4
    assert lib.sf_lstm_weights_bf16(None, None, p, p) == ERR_ARG
    assert lib.sf_lstm_weights_bf16(p, p, p, None) == ERR_ARG              # a second weight needs its packed image
    assert lib.sf_lstm_weights_bf16(p, None, p, p) == ERR_ARG              # ... and no image without the weight
    assert lib.sf_lstm_weights_bf16(p, p, None, p) == ERR_ARG
    # the table: a pair registers, re-registers, is forgotten (twice: the second time there is nothing to forget)
    assert lib.sf_lstm_weights_bf16(p, p, p, p) == 0
    assert lib.sf_lstm_weights_bf16(p, p, p, p) == 0
    assert lib.sf_lstm_weights_bf16(p, p, None, None) == 0
    assert lib.sf_lstm_weights_bf16(p, p, None, None) == 0
    # 16 pairs fit, the 17th is refused, forgetting one makes room
    keys = [C.c_void_p(p.value + 4 * i) for i in range(17)]
    try:
        for k in keys[:16]:
            assert lib.sf_lstm_weights_bf16(k, None, p, None) == 0
        assert lib.sf_lstm_weights_bf16(keys[16], None, p, None) == 2      # SF_ERR_UNSUPPORTED
        assert lib.sf_lstm_weights_bf16(keys[0], None, None, None) == 0
        assert lib.sf_lstm_weights_bf16(keys[16], None, p, None) == 0
    finally:
        for k in keys:
            lib.sf_lstm_weights_bf16(k, None, None, None)


def test_switch_reads_back_and_the_strict_switch_is_its_own():
    from speaker_follower_amd import runtime
    from speaker_follower_amd._lib import lib
    assert lib.sf_gate_product_bf16_weights_is_on() == 0                   # off by default
    with runtime.bf16_gate_weights():
        assert lib.sf_gate_product_bf16_weights_is_on() == 1
        with runtime.bf16_gate_weights(False):
            assert lib.sf_gate_product_bf16_weights_is_on() == 0
        assert lib.sf_gate_product_bf16_weights_is_on() == 1
        # the strict switch is independent of it (and wins where a product is launched: tests/test_gpu_gate_bf16.py)
        with runtime.strict_gate_product():
            assert lib.sf_gate_product_is_strict() == 1 and lib.sf_gate_product_bf16_weights_is_on() == 1
        assert lib.sf_gate_product_is_strict() == 0
    assert lib.sf_gate_product_bf16_weights_is_on() == 0
    with pytest.raises(RuntimeError):
        with runtime.bf16_gate_weights():
            raise RuntimeError('inside')
    assert lib.sf_gate_product_bf16_weights_is_on() == 0                   # restored on the way out of an exception


def test_gate_weights_takes_its_two_values_only():
    from speaker_follower_amd import agents, follower, runtime, search
    eng = follower.FollowerEngine(None, None, None)
    agent = agents.Seq2SeqAgent(None, '/tmp/sf_gate_bf16.json', None, None)
    assert eng.gate_weights == 'fp32' and agent.gate_weights == 'fp32'
    for obj in (eng, agent):
        obj.gate_weights = 'bf16'
        assert obj.gate_weights == 'bf16'
        for bad in ('fp16', 'BF16', '', None, 1, True, b'bf16'):
            with pytest.raises(ValueError):
                obj.gate_weights = bad
        assert obj.gate_weights == 'bf16'                                  # a refused value changes nothing
        obj.gate_weights = 'fp32'
    # the agent hands its mode to the engines it holds
    agent._engine = follower.FollowerEngine(None, None, None)
    agent._score_engine = follower.FollowerEngine(None, None, None)
    agent.gate_weights = 'bf16'
    assert agent._engine.gate_weights == agent._score_engine.gate_weights == 'bf16'
    with pytest.raises(ValueError):
        runtime.check_gate_weights('int8')
    for cls in (search.FlatDecoder, search.GraphStep, search.DeviceFollowerBeam):
        with pytest.raises(ValueError):
            cls(*([None] * (4 if cls is search.FlatDecoder else 6 if cls is search.GraphStep else 7)), gate_weights='fp16')


def test_cache_keys_of_captured_inference_graphs_include_the_mode():
    from speaker_follower_amd import agents, follower, runtime, search
    agent = agents.Seq2SeqAgent(None, '/tmp/sf_gate_bf16.json', object(), object())
    agent.store = object()
    nav = object()
    eng = follower.FollowerEngine(None, None, None)
    keys = {}
    for mode in ('fp32', 'bf16'):
        eng.gate_weights = mode
        keys[mode] = (search.graph_step_key(agent, nav, 8, 16, 80, mode),
                      search.follower_beam_key(agent, nav, 8, 3, 80, 2, True, mode),
                      agent._test_graph_key(nav, eng, 8),
                      runtime.gate_mode_key(mode))
    for a, b in zip(keys['fp32'], keys['bf16']):
        assert a != b and a[:-2] == b[:-2] and (a[-2], b[-2]) == ('fp32', 'bf16') and a[-1] == b[-1] == 0
    # ... and the strict switch, as before: the key's last element
    with runtime.strict_gate_product():
        strict = search.graph_step_key(agent, nav, 8, 16, 80, 'fp32')
        strict_beam = search.follower_beam_key(agent, nav, 8, 3, 80, 2, True, 'fp32')
    assert strict[-1] == 1 and strict[:-1] == keys['fp32'][0][:-1]
    assert strict_beam[-1] == 1 and strict_beam[:-1] == keys['fp32'][1][:-1]
    with pytest.raises(ValueError):
        search.graph_step_key(agent, nav, 8, 16, 80, 'fp64')


def test_a_taped_pass_is_always_an_fp32_pass():
    """FollowerEngine.pass_gate_weights: train mode, or parameters that require grad under grad mode, ignore the attribute."""
    import torch
    from speaker_follower_amd import follower
    enc, dec = torch.nn.Linear(2, 2), torch.nn.Linear(2, 2)
    eng = follower.FollowerEngine(enc, dec, None)
    eng.gate_weights = 'bf16'
    dec.eval()
    assert eng.pass_gate_weights(train=True) == 'fp32'
    assert eng.pass_gate_weights(train=False) == 'fp32'                    # grad mode on, parameters require grad: a tape
    with torch.no_grad():
        assert eng.pass_gate_weights(train=False) == 'bf16'
        assert eng.pass_gate_weights() == 'bf16'                           # (train=None: the module's own mode, eval)
        assert eng.pass_gate_weights(train=True) == 'fp32'
        dec.train()
        assert eng.pass_gate_weights() == 'fp32'
    dec.eval()
    for p in list(enc.parameters()) + list(dec.parameters()):
        p.requires_grad_(False)
    assert eng.pass_gate_weights(train=False) == 'bf16'                    # nothing to differentiate: inference
    eng.gate_weights = 'fp32'
    assert eng.pass_gate_weights(train=False) == 'fp32'
