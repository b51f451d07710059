"""CPU: the host side of follower pre-training on a routes.RouteSet -- DeviceNavBatch.pack_layout,
RouteSet.follower_minibatch_host against env._next_minibatch(sort=True) + DeviceNavBatch.host_arrays_for(fixed=True) on
the eight committed connectivity graphs, the numpy restatement of sf_nav_follower_batches
(tests/follower_pack_cases.py) against the same function so that it is pinned before the kernel is held to it
(tests/test_gpu_follower_batches.py), epoch_order, with_generated and the refusals.  Every comparison is ==."""
import json
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import follower_pack_cases as F                                     # noqa: E402
import nav_route_cases as R                                         # noqa: E402

ROOT = os.path.dirname(HERE)
KEYS = ('seq', 'mask', 'lengths', 'rows', 'views', 'hop', 'base')
PAD, EOS = 0, 2


@pytest.fixture(scope='module')
def world():
    from speaker_follower_amd.routes import RouteSet
    env, nav, dist, _ = R.fixture_world()
    fx = json.load(open(os.path.join(HERE, 'golden', 'r2r_fixture_items.json')))['items']
    return dict(env=env, nav=nav, routes=RouteSet.enumerate(nav, dist), split=fx)


def test_the_header_declares_the_entry_and_the_library_binds_it():
    from speaker_follower_amd import _cdecl, _lib
    text = open(os.path.join(ROOT, 'include', 'sf_hip.h')).read()
    h = _cdecl.parse(text)
    assert re.search(r'^int sf_nav_follower_batches\(const sf_nav_follower_io\* io, int32_t\* err, sf_stream stream\);$',
                     text, re.M)
    assert [p[0] for p in h.functions['sf_nav_follower_batches'].params] == ['io', 'err', 'stream']
    fields = dict(h.structs)['sf_nav_follower_io']
    assert [f[0] for f in fields] == [n for n, _ in _lib.NavFollowerIO._fields_] and len(fields) == 24
    assert _lib.STRUCTS['sf_nav_follower_io'] is _lib.NavFollowerIO
    assert 'sf_nav_follower_batches' in _lib.EXPORTS and _lib.lib.sf_nav_follower_batches_max_b() >= 1024
    assert _lib.ABI_VERSION == 10                                     # (additive: the version stays)


def test_pack_layout_offsets():
    from speaker_follower_amd.nav import DeviceNavBatch
    want = {(1, 1, 1): dict(seq=(0, 8), mask=(64, 1), lengths=(128, 4), rows=(192, 4), views=(256, 4), hop=(320, 4),
                            base=(384, 4), bytes=448),
            (5, 8, 3): dict(seq=(0, 320), mask=(320, 40), lengths=(384, 20), rows=(448, 20), views=(512, 20), hop=(576, 60),
                            base=(640, 20), bytes=704),
            (100, 80, 345): dict(seq=(0, 64000), mask=(64000, 8000), lengths=(72000, 400), rows=(72448, 400),
                                 views=(72896, 400), hop=(73344, 138000), base=(211392, 400), bytes=211840)}
    for shape, lay in want.items():
        got = DeviceNavBatch.pack_layout(*shape)
        assert got == lay and list(got) == list(KEYS) + ['bytes']     # (in _LOADED order)
        assert got == F.layout(*shape)
        assert all(v[0] % 64 == 0 for k, v in got.items() if k != 'bytes') and got['bytes'] % 64 == 0
    assert [k for _, k in DeviceNavBatch._LOADED] == list(KEYS)


def host_path(nav, items, Lmax, reverse):
    """What the training loop forms today: the environment's sort, then host_arrays_for of the sorted items."""
    from speaker_follower_amd.nav import DeviceNavBatch
    ordered = sorted(items, key=lambda it: len(it['instr_encoding']), reverse=True)
    return DeviceNavBatch.host_arrays_for(nav, ordered, Lmax, reverse, fixed=True), ordered


def same_minibatch(got, want):
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert (got[k] == want[k]).all(), k
        assert got[k].flags['C_CONTIGUOUS'], k


@pytest.mark.parametrize('reverse', [True, False])
def test_the_host_minibatch_equals_the_environments_on_the_committed_split(world, reverse):
    from speaker_follower_amd.routes import RouteSet
    nav, split = world['nav'], world['split']
    rs = RouteSet.from_items(nav, split)
    rng = np.random.default_rng(5)
    assert len({len(it['instr_encoding']) for it in split}) > 3
    for B, Lmax in ((1, 80), (7, 80), (len(split), 80), (7, 14), (5, 1), (6, 2)):
        for _ in range(3):
            idx = rng.permutation(len(split))[:B]
            got = rs.follower_minibatch_host(idx, Lmax, reverse=reverse)
            want, ordered = host_path(nav, [split[i] for i in idx], Lmax, reverse)
            same_minibatch(got, want)
            assert [split[r]['instr_id'] for r in got['route']] == [it['instr_id'] for it in ordered]
            assert got['hop'].shape[1] == max(nav.scan_rows.values())


def enumerated_with_tokens(world, n, seed, lens=None):
    rng = np.random.default_rng(seed)
    rs = world['routes'].sample(n, seed)
    lens = rng.integers(0, 19, n) if lens is None else lens          # (many equal lengths among 200; 0 and above Lmax = 14)
    tokens, off = F.tokens_of(rng, lens)
    enc = F.encodings(tokens, off)
    items = [dict(it, instr_encoding=e) for it, e in zip(rs.items(), enc)]
    return rs.with_instructions(enc), items, (tokens, off)


def test_the_host_minibatch_equals_the_environments_on_enumerated_routes(world):
    rs, items, _ = enumerated_with_tokens(world, 200, 21)
    rng = np.random.default_rng(22)
    raw = np.array([len(e) for e in rs.enc])
    assert len(set(raw.tolist())) < 25 and raw.min() == 0 and raw.max() > 14
    for B in (1, 2, 63, 100, 200):
        idx = rng.permutation(200)[:B]
        got = rs.follower_minibatch_host(idx, 14, reverse=True)
        want, ordered = host_path(world['nav'], [items[i] for i in idx], 14, True)
        same_minibatch(got, want)
        assert [items[r]['instr_id'] for r in got['route']] == [it['instr_id'] for it in ordered]
    twice = np.array([3, 9, 3, 3, 9])                                  # a route drawn more than once
    same_minibatch(rs.follower_minibatch_host(twice, 14), host_path(world['nav'], [items[i] for i in twice], 14, True)[0])
    with pytest.raises(AssertionError):                                # the host path's own assertion
        rs.with_instructions([[5, EOS]] * 200).follower_minibatch_host([0], 14)


def route_arrays(rs):
    return dict(row0=rs.row0, view0=rs.view0, hop_all=rs.nav.all_hops(), hop_off=rs.hop_off, hop_base=rs.hop_base,
                hop_rows=rs.hop_rows)


@pytest.mark.parametrize('reverse', [True, False])
def test_the_restatement_equals_the_host_minibatch(world, reverse):
    rs, items, (tokens, off) = enumerated_with_tokens(world, 200, 31)
    rng = np.random.default_rng(32)
    ld = max(world['nav'].scan_rows.values())
    for B, Lmax, M in ((1, 1, 2), (7, 14, 3), (100, 14, 2), (65, 8, 3)):
        order = rng.integers(0, 200, M * B).astype(np.int32)
        nbytes = F.layout(B, Lmax, ld)['bytes']
        mb_off = np.arange(M) * (nbytes + 64)
        before = np.full(M * (nbytes + 64), 0x5A, np.uint8)
        got = F.mirror_follower(route_arrays(rs), order, B, Lmax, ld, 36, mb_off, before, tokens, off, reverse=reverse)
        assert got['err'] == 0
        free = F.gap_mask(B, Lmax, ld, mb_off, len(before))
        assert (got['out'][free] == 0x5A).all() and free[-64:].all()
        for i in range(M):
            want = rs.follower_minibatch_host(order[i * B:(i + 1) * B], Lmax, reverse=reverse)
            sec = F.sections(got['out'][mb_off[i]:mb_off[i] + nbytes], B, Lmax, ld)
            for k in KEYS:
                assert (sec[k] == want[k]).all(), (k, i)
            assert (got['col_route'][i] == want['route']).all() and (got['col_len'][i] == want['lengths']).all()
    # no tokens at all: every instruction is [EOS]
    got = F.mirror_follower(route_arrays(rs), np.arange(5, dtype=np.int32), 5, 3, ld, 36, [0],
                            np.zeros(F.layout(5, 3, ld)['bytes'], np.uint8), reverse=reverse)
    want = world['routes'].sample(200, 31).follower_minibatch_host(np.arange(5), 3, reverse=reverse)
    sec = F.sections(got['out'], 5, 3, ld)
    assert all((sec[k] == want[k]).all() for k in KEYS) and (sec['seq'] == [[EOS, PAD, PAD]] * 5).all()


def test_epoch_order(world):
    rs = world['routes'].sample(50, 1)
    order = rs.epoch_order(7, 17, seed=3)                              # 119 slots: two epochs and 19 of the third
    assert order.dtype == np.int32 and order.shape == (119,)
    assert sorted(order[:50].tolist()) == sorted(order[50:100].tolist()) == list(range(50))
    assert len(set(order[100:].tolist())) == 19
    assert order[:50].tolist() != order[50:100].tolist()
    assert (order[:50] == np.random.default_rng([3, 0]).permutation(50)).all()
    assert (order[100:] == np.random.default_rng([3, 2]).permutation(50)[:19]).all()
    assert (rs.epoch_order(7, 17, seed=3) == order).all() and (rs.epoch_order(7, 17, seed=4) != order).any()
    assert (rs.epoch_order(7, 3, seed=3) == order[:21]).all()          # a cut that falls inside the first epoch
    assert len(rs.epoch_order(7, 0)) == 0


class _Tokenizer:
    """The reference's Tokenizer as far as with_generated uses it: ids 0 .. 3 are <PAD>, <UNK>, <EOS>, <BOS>."""
    vocab = ['<PAD>', '<UNK>', '<EOS>', '<BOS>', 'walk', 'left', 'stairs']

    def decode_sentence(self, encoding, break_on_eos=False, join=True):
        words = []
        for ix in encoding:
            if ix == (EOS if break_on_eos else PAD):
                break
            words.append(self.vocab[ix])
        return ' '.join(words) if join else words

    def encode_sentence(self, sentence):
        words = [w for w in re.split(r'(\W+)', sentence.strip().lower()) if w.strip()]      # ('<unk>' splits into '<', 'unk', '>')
        enc = [self.vocab.index(w) if w in self.vocab else 1 for w in (x.strip() for x in words)]
        return np.array(enc), len(enc)


def test_with_generated_cuts_at_eos_and_counts_ids_that_do_not_round_trip(world):
    rs = world['routes'].sample(5, 2)
    words = [[4, 5, EOS, 6, 6], [4, 5, 6], [EOS, 4], [4, 1, 5, EOS, PAD], [3, 4, EOS]]
    results = {k: {'word_indices': w} for k, w in zip(rs.instr_ids, words)}
    results = dict(reversed(list(results.items())))                    # (looked up by instr_id, not by position)
    out = rs.with_generated(results)
    assert [e.tolist() for e in out.enc] == [[4, 5], [4, 5, 6], [], [4, 1, 5], [3, 4]]
    assert all(e.dtype == np.int64 for e in out.enc) and rs.enc is None
    assert out.nav is rs.nav and (out.row0 == rs.row0).all() and out.instr_ids == rs.instr_ids
    again, odd = rs.with_generated(results, tokenizer=_Tokenizer())
    assert [e.tolist() for e in again.enc] == [e.tolist() for e in out.enc] and odd == 2      # <UNK> in one, <BOS> in another
    mb = out.follower_minibatch_host(np.arange(5), 4)
    assert mb['route'].tolist() == [1, 3, 0, 4, 2] and mb['lengths'].tolist() == [4, 4, 3, 3, 1]
    assert mb['seq'].tolist() == [[6, 5, 4, EOS], [5, 1, 4, EOS], [5, 4, EOS, PAD], [4, 3, EOS, PAD], [EOS, PAD, PAD, PAD]]


def test_refusals(world):
    rs = world['routes'].sample(20, 3)
    with pytest.raises(ValueError):
        rs.with_instructions([[4]] * 19)
    with pytest.raises(ValueError):
        rs.pack_follower(7, 14, order=np.arange(20))                   # not a whole number of minibatches
    with pytest.raises(ValueError):
        rs.pack_follower(7, 14, order=np.arange(0))
    with pytest.raises(ValueError):
        rs.follower_windows(7, 14, np.arange(20))
    w = rs.follower_windows(7, 14, np.arange(21) % 20, window=2)       # (nothing is packed before a block is asked for)
    assert len(w) == 3 and w.packed == 0 and w.window == 2
    with pytest.raises(ValueError):
        rs.take([]).epoch_order(7, 2)
