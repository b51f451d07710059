"""GPU, end to end on the eight committed scans: RouteSet.pack_follower (sf_nav_follower_batches) against
RouteSet.follower_minibatch_host (pinned to the environment's host path by tests/test_follower_routes_host.py), section
by section with the gaps untouched; DeviceNavBatch.load_packed against load(items); and Seq2SeqAgent.train_on_routes
against train() over an environment of the same items -- the same graph over the same bytes, so losses and weights are
compared with ==."""
import copy
import os
import random
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import follower_pack_cases as F                                     # noqa: E402
import nav_route_cases as R                                         # noqa: E402
from speaker_follower_amd import synth                              # noqa: E402

LMAX, EPISODE, FILL = 14, 4, 0x5A
KEYS = F.SECTIONS


@pytest.fixture(scope='module')
def world():
    from speaker_follower_amd import features
    from speaker_follower_amd.routes import RouteSet
    state = random.getstate()
    env, nav, dist, n_rows = R.fixture_world('cuda')
    routes = RouteSet.enumerate(nav, dist)
    rng = np.random.default_rng(41)
    tokens, off = F.tokens_of(rng, rng.integers(0, LMAX + 5, len(routes)), lo=4, hi=synth.FULL.vocab)
    enc = F.encodings(tokens, off)
    items = [dict(it, instr_encoding=e) for it, e in zip(routes.items(), enc)]
    yield dict(base=env, nav=nav, routes=routes.with_instructions(enc), items=items,
               store=features.FeatureStore(synth.feature_table(21, n_rows)))
    random.setstate(state)


@pytest.fixture
def filled_buffers(monkeypatch):
    """Every uint8 buffer torch.empty hands out holds FILL: what pack_follower does not write stays visible."""
    real = torch.empty

    def empty(*a, **k):
        t = real(*a, **k)
        return t.fill_(FILL) if t.dtype == torch.uint8 else t
    monkeypatch.setattr(torch, 'empty', empty)


@pytest.mark.parametrize('B,chunk', [(100, 2), (100, None), (7, 2), (7, None)])
def test_pack_follower_equals_the_host_minibatches(world, filled_buffers, B, chunk):
    rs = world['routes']
    assert len(rs) == 1734
    ld = max(world['nav'].scan_rows.values())
    for order in (None, rs.epoch_order(B, 20, seed=B)):
        blocks = rs.pack_follower(B, LMAX, order=order, chunk=chunk)
        drawn = np.arange(-(-1734 // B) * B) % 1734 if order is None else order
        M = len(drawn) // B
        per = chunk or M
        assert len(blocks) == M and (blocks.B, blocks.Lmax, blocks.ld) == (B, LMAX, ld)
        assert len({b[0].data_ptr() for b in blocks.blocks}) == -(-M // per)          # a buffer per chunk
        assert blocks.col_route.shape == blocks.col_len.shape == (M, B) and blocks.col_route.dtype == np.int32
        free = F.gap_mask(B, LMAX, ld, [0], blocks.bytes)
        host = {b[0].data_ptr(): b[0].cpu().numpy() for b in blocks.blocks}
        for i in range(M):
            buf, off = blocks.blocks[i]
            blk = host[buf.data_ptr()][off:off + blocks.bytes]
            assert (blocks.block(i).cpu().numpy() == blk).all() if i in (0, M - 1) else True
            want = rs.follower_minibatch_host(drawn[i * B:(i + 1) * B], LMAX)
            sec = F.sections(blk, B, LMAX, ld)
            for k in KEYS:
                assert sec[k].dtype == want[k].dtype and (sec[k] == want[k]).all(), (k, i)
            assert (blk[free] == FILL).all() and free.any(), i
            assert (blocks.col_route[i] == want['route']).all() and (blocks.col_len[i] == want['lengths']).all()
    with pytest.raises(ValueError):
        rs.pack_follower(B, LMAX, order=np.arange(B + 1))
    with pytest.raises(RuntimeError):
        rs.pack_follower(B, LMAX, order=np.full(B, 1734))


def test_load_packed_leaves_what_load_of_the_sorted_items_leaves(world):
    from speaker_follower_amd.nav import DeviceNavBatch
    rs, nav, items = world['routes'], world['nav'], world['items']
    B = 7
    order = rs.epoch_order(B, 6, seed=2)
    blocks = rs.pack_follower(B, LMAX, order=order)
    mine, theirs = (DeviceNavBatch(nav, items[:B], EPISODE, max_length=LMAX, fixed_shapes=True) for _ in range(2))
    for i in (3, 0, 5):
        drawn = [items[r] for r in order[i * B:(i + 1) * B]]
        ordered = sorted(drawn, key=lambda it: len(it['instr_encoding']), reverse=True)
        theirs.load(ordered)
        mine.load_packed(blocks, i)
        torch.cuda.synchronize()
        for attr, _ in DeviceNavBatch._LOADED:
            a, b = getattr(mine, attr), getattr(theirs, attr)
            assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), (attr, i)
        assert mine.lengths == theirs.lengths
        assert [items[r]['instr_id'] for r in mine.items] == [it['instr_id'] for it in ordered]
    with pytest.raises(ValueError):
        mine.load_packed(rs.pack_follower(B, LMAX - 1, order=order), 0)
    with pytest.raises(ValueError):
        mine.load_packed(rs.pack_follower(B + 1, LMAX, order=np.arange(B + 1)), 0)
    loose = DeviceNavBatch(nav, items[:B], EPISODE, max_length=LMAX)
    with pytest.raises(ValueError):
        loose.load_packed(blocks, 0)


def fresh_agent(world, env):
    from speaker_follower_amd import agents, model, optim
    d = synth.FULL
    enc_w, dec_w = synth.follower_weights_peaky(303)
    enc = model.EncoderLSTM(d.vocab, d.word, d.hidden, 0, 0.5, glove=enc_w['embedding.weight'])
    dec = model.AttnDecoderLSTM(d.feat, d.hidden, 0.5, feature_size=d.feat)
    enc.load_state_dict({k: torch.tensor(v) for k, v in enc_w.items()})
    dec.load_state_dict({k: torch.tensor(v) for k, v in dec_w.items()})
    enc.cuda()
    dec.cuda()
    torch.manual_seed(4)
    ag = agents.Seq2SeqAgent(env, '/tmp/sf_follower_routes.json', enc, dec, episode_len=EPISODE, max_instruction_length=LMAX)
    ag.store = world['store']
    ag.use_device_env(world['nav'])
    oe = optim.FusedAdam([p for p in enc.parameters() if p.requires_grad], lr=1e-4, weight_decay=5e-4)
    od = optim.FusedAdam([p for p in dec.parameters() if p.requires_grad], lr=1e-4, weight_decay=5e-4)
    return ag, oe, od, [p for m in (enc, dec) for p in m.parameters()]


def test_train_on_routes_equals_train_over_an_environment_of_the_same_items(world, monkeypatch):
    from speaker_follower_amd import env as E
    from speaker_follower_amd.nav import DeviceNavBatch
    B, n = 7, 3
    rs, base = world['routes'], world['base']
    items = world['items'][:B * n]
    assert len({len(it['instr_encoding']) for it in items}) < len(items)          # (equal lengths among them)
    env = E.R2RIndexEnv(items, base.row_of, base.nav_graph_path, batch_size=B, scans=world['nav'].scans)
    env.data[:] = items                                                # the routes' order: no shuffle, and 21 = 3 x 7: no wrap
    env.reset_epoch()
    a, oe, od, pa = fresh_agent(world, env)
    a.train(oe, od, n, feedback='teacher')
    assert a._train_graph_state[1].replays == n - 1
    b, oe2, od2, pb = fresh_agent(world, env)
    b.env = None                                                       # no environment involved
    with monkeypatch.context() as m:
        refuse = lambda *args, **kw: pytest.fail('the host path of a minibatch ran')            # noqa: E731
        m.setattr(DeviceNavBatch, 'host_arrays_for', staticmethod(refuse))
        m.setattr(DeviceNavBatch, 'load', refuse)
        packs, pack = [], type(rs).pack_follower
        m.setattr(type(rs), 'pack_follower', lambda self, *a, **k: packs.append(len(k['order'])) or pack(self, *a, **k))
        b.route_window = 2                                             # (three iterations: a window of two and one of one)
        b.train_on_routes(rs, oe2, od2, n, feedback='teacher', batch_size=B, order=np.arange(B * n))
        assert packs == [2 * B, B]
        b.route_window = None
    print('[train_on_routes] losses', b.losses, 'train()', a.losses)
    assert len(b.losses) == n and b.losses == a.losses and len(set(b.losses)) == n
    assert float(b.loss) == b.losses[-1]
    assert all(torch.equal(x, y) for x, y in zip(pa, pb))
    assert b._train_graph_state[1].replays == n - 1 and oe2.host_steps() == oe.host_steps() == [n]
    # the graph train() captured serves train_on_routes too (same optimizers, feedback, table, batch size)
    tg = a._train_graph_state[1]
    a.train_on_routes(rs, oe, od, 2, batch_size=B, order=np.arange(B, 3 * B))
    b.train_on_routes(rs, oe2, od2, 2, batch_size=B, order=np.arange(B, 3 * B))
    assert a._train_graph_state[1] is tg and tg.replays == n + 1
    assert a.losses == b.losses and len(a.losses) == 2 and all(torch.equal(x, y) for x, y in zip(pa, pb))
    # the default order is epoch_order(batch_size, n_iters, seed)
    b.train_on_routes(rs, oe2, od2, 2, batch_size=B, seed=5)
    a.train_on_routes(rs, oe, od, 2, batch_size=B, order=rs.epoch_order(B, 2, 5))
    assert a.losses == b.losses and len(b.losses) == 2
    # what cannot be replayed, and routes over another table
    other = copy.copy(rs)
    other.nav = copy.copy(rs.nav)
    with pytest.raises(ValueError):
        b.train_on_routes(other, oe2, od2, 1, batch_size=B)
    with pytest.raises(ValueError):
        b.train_on_routes(rs, oe2, od2, 2, batch_size=B, order=np.arange(B))
    with pytest.raises(NotImplementedError, match="'\\+' feedback"):
        b.train_on_routes(rs, oe2, od2, 1, feedback='teacher+sample', batch_size=B)
    # a process group is refused whatever else holds -- also the one configuration train() replays in segments
    for group, sync in ((object(), object()), (object(), None), (None, object())):
        b._engine.group, b._engine.grad_sync = group, sync
        try:
            with pytest.raises(NotImplementedError, match='a process group'):
                b.train_on_routes(rs, oe2, od2, 1, batch_size=B)
            with pytest.raises(NotImplementedError, match='a process group'):
                b.train_on_routes(rs, torch.optim.SGD(pb[:1], lr=0.1), od2, 1, batch_size=B)
        finally:
            b._engine.group = b._engine.grad_sync = None
    sgd = torch.optim.SGD(pb[:1], lr=0.1)
    with pytest.raises(NotImplementedError, match='optimizer'):
        b.train_on_routes(rs, sgd, od2, 1, batch_size=B)
    assert all(torch.equal(x, y) for x, y in zip(pa, pb))
