"""CPU: routes.RouteSet and NavTable.all_hops on the eight committed connectivity graphs, and the numpy mirror of
sf_nav_routes (tests/nav_route_cases.py) against the host path -- NavTable.gold_routes -> Seq2SeqSpeaker._index_batch ->
speaker.pack_speaker_batch -- section by section, so that the mirror is pinned before the kernel is held to it
(tests/test_gpu_nav_routes.py).  Every comparison is ==."""
import json
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import nav_route_cases as R                                         # noqa: E402

ROOT = os.path.dirname(HERE)
COUNTS = {'17DRP5sb8fy': 382, '2t7WUuJeko7': 600, '8194nk5LbLH': 104, 'GdvgFV5R1Z5': 28, 'Pm6F8kyY3z2': 240,
          'YmJkqBEsHnH': 36, 'gZ6f7yhEvPG': 0, 'pLe4wQe7qrG': 344}
SHORT_OF_5M = {'17DRP5sb8fy': 68, '2t7WUuJeko7': 14, 'Pm6F8kyY3z2': 36, 'pLe4wQe7qrG': 14}
S, LMAX = 10, 12


@pytest.fixture(scope='module')
def world():
    from speaker_follower_amd.routes import RouteSet
    env, nav, dist, _ = R.fixture_world()
    routes = RouteSet.enumerate(nav, dist)
    return dict(env=env, nav=nav, dist=dist, routes=routes, items=routes.items())


def test_the_header_declares_the_entry_and_the_library_binds_it():
    from speaker_follower_amd import _cdecl, _lib
    text = open(os.path.join(ROOT, 'include', 'sf_hip.h')).read()
    h = _cdecl.parse(text)
    assert re.search(r'^int sf_nav_routes\(const sf_nav_table\* nav, const sf_nav_routes_io\* io, int32_t\* err, '
                     r'sf_stream stream\);$', text, re.M)
    assert [p[0] for p in h.functions['sf_nav_routes'].params] == ['nav', 'io', 'err', 'stream']
    fields = dict(h.structs)['sf_nav_routes_io']
    assert [f[0] for f in fields] == [n for n, _ in _lib.NavRoutesIO._fields_] and len(fields) == 27
    assert 'sf_nav_routes' in _lib.EXPORTS and len(_lib.lib.sf_nav_routes.argtypes) == 4
    assert _lib.STRUCTS['sf_nav_routes_io'] is _lib.NavRoutesIO
    assert _lib.ABI_VERSION == 10                                     # (additive: the version stays)


def test_all_hops_stacks_the_hop_rows_of_every_goal(world):
    nav = world['nav']
    hop = nav.all_hops()
    assert hop.dtype == np.int32 and hop.ndim == 1 and len(hop) == sum(m * m for m in nav.scan_rows.values())
    assert len(hop) == len(world['dist'].host)                        # as many elements as the distance table
    for s in nav.scans:
        b, m, o = nav.base[s], nav.scan_rows[s], nav.hop_off[s]
        for g in range(m):
            want = nav.hops(s, nav.vp_of[b + g][1])
            assert (hop[o + g * m:o + (g + 1) * m] == want).all(), (s, g)
            assert hop[o + g * m + g] == b + g                        # the goal points at itself
    assert nav.all_hops() is hop                                      # built once


def test_enumeration_counts_and_order(world):
    nav, rs, dist = world['nav'], world['routes'], world['dist']
    assert len(rs) == 1734 and rs.unreached == 0
    per_scan = np.bincount(rs.scan_ix, minlength=len(nav.scans))
    assert {s: int(per_scan[i]) for i, s in enumerate(nav.scans)} == COUNTS
    key = list(zip(rs.scan_ix.tolist(), rs.row0.tolist(), rs.goal.tolist()))
    assert key == sorted(key) and len(set(key)) == len(key)           # scan, then start row, then goal row
    n, rows = rs.walked
    assert np.bincount(n).tolist() == [0, 0, 0, 0, 0, 706, 594, 434]
    assert (rs.distance >= 5.0).all()
    # the metre rule bites: pairs with 4 .. 6 hops that fall below 5 m
    from speaker_follower_amd.routes import RouteSet
    loose = RouteSet.enumerate(nav, dist, min_metres=0.0)
    extra = np.bincount(loose.scan_ix, minlength=len(nav.scans)) - per_scan
    assert {s: int(extra[i]) for i, s in enumerate(nav.scans) if extra[i]} == SHORT_OF_5M
    # ... and so does the hop rule, and `scans` restricts
    assert len(RouteSet.enumerate(nav, dist, min_hops=1, max_hops=6)) > len(rs)
    one = RouteSet.enumerate(nav, dist, scans={'GdvgFV5R1Z5'})
    assert len(one) == 28 and set(one.scan_ix.tolist()) == {nav.scans.index('GdvgFV5R1Z5')}


def test_enumeration_matches_the_graphs_own_paths_and_distances(world):
    env, nav, rs = world['env'], world['nav'], world['routes']
    n, rows = rs.walked
    for i, it in enumerate(world['items']):
        g = env.graphs[it['scan']]
        start, goal = nav.vp_of[rs.row0[i]][1], nav.vp_of[rs.goal[i]][1]
        assert it['path'] == g.path(start, goal), i
        assert 4 <= len(it['path']) - 1 <= 6 and n[i] == len(it['path'])
        assert it['distance'] == world['dist'].block(it['scan'])[rs.row0[i] - nav.base[it['scan']],
                                                                  rs.goal[i] - nav.base[it['scan']]]
        assert it['distance'] == pytest.approx(g.distance(start, goal), rel=1e-12) and it['distance'] >= 5.0
        assert it['instr_id'] == '%d_0' % it['path_id'] and it['instructions'] == [''] and it['instr_encoding'] == []
    assert [it['path_id'] for it in world['items']] == list(range(1734))
    assert [it['path_id'] for it in rs.items(first_path_id=50)][:2] == [50, 51]


def line_world(edge):
    """Rows 0 .. 5 on a line with edges `edge` metres long, rows 6 and 7 a component of their own."""
    m = 8
    hop = np.zeros((m, m), np.int32)
    D = np.full((m, m), np.inf)
    for g in range(m):
        for r in range(m):
            same = (g < 6) == (r < 6)
            hop[g, r] = r + (g > r) - (g < r) if same else r
            if same:
                D[r, g] = sum(edge[min(r, g):max(r, g)]) if g < 6 else abs(g - r) * 1.0
    vp = ['v%d' % i for i in range(m)]
    nav = types.SimpleNamespace(scans=['L'], scan_rows={'L': m}, base={'L': 0}, hop_off={'L': 0},
                                vp_of=[('L', v) for v in vp], all_hops=lambda: hop.reshape(-1), device=torch.device('cpu'))
    # candidate tables of the line: slot 1 leads up, slot 2 down (nav_walk_cases.line_table), per component
    import nav_walk_cases as W
    a, b = W.line_table(6, 36, 3), W.line_table(2, 36, 3)
    nav.host = dict(a_num=np.concatenate([a['a_num'], b['a_num']]),
                    next_row=np.concatenate([a['next_row'], b['next_row'] + 6]),
                    cand_view=np.concatenate([a['cand_view'], b['cand_view']]))
    dist = types.SimpleNamespace(nodes={'L': vp}, block=lambda s: D)
    return nav, dist


def test_enumeration_on_a_line_graph_each_limit_excludes_a_pair():
    from speaker_follower_amd.routes import RouteSet
    nav, dist = line_world([2.0, 2.0, 2.0, 2.0, 0.5])
    pairs = lambda rs: sorted(zip(rs.row0.tolist(), rs.goal.tolist()))          # noqa: E731
    # 4 .. 6 hops and >= 5 m: 0 <-> 4 (8 m), 0 <-> 5 (8.5 m), 1 <-> 5 (6.5 m)
    assert pairs(RouteSet.enumerate(nav, dist)) == [(0, 4), (0, 5), (1, 5), (4, 0), (5, 0), (5, 1)]
    # the hop ceiling excludes the five-hop pair, the hop floor the four-hop ones
    assert pairs(RouteSet.enumerate(nav, dist, max_hops=4)) == [(0, 4), (1, 5), (4, 0), (5, 1)]
    assert pairs(RouteSet.enumerate(nav, dist, min_hops=5)) == [(0, 5), (5, 0)]
    # the metre limit excludes 1 <-> 5 (6.5 m) and keeps the others
    assert pairs(RouteSet.enumerate(nav, dist, min_metres=7.0)) == [(0, 4), (0, 5), (4, 0), (5, 0)]
    # nothing leads into or out of the other component, whatever the limits
    everything = RouteSet.enumerate(nav, dist, min_hops=1, max_hops=7, min_metres=0.0)
    assert pairs(everything) == sorted([(a, b) for a in range(6) for b in range(6) if a != b] + [(6, 7), (7, 6)])
    assert everything.unreached == 0


def test_sampling_and_headings(world):
    from speaker_follower_amd.env import ANGLE_INC, snapped_view
    rs = world['routes']
    k = np.random.default_rng(0).integers(12, size=len(rs))
    assert (rs.heading == k * ANGLE_INC).all() and (rs.view0 == 12 + k).all()
    assert [snapped_view(h) for h in rs.heading.tolist()] == rs.view0.tolist()
    a, b, c = rs.sample(200, 3), rs.sample(200, 3), rs.sample(200, 4)
    key = lambda x: list(zip(x.row0.tolist(), x.goal.tolist()))                 # noqa: E731
    assert key(a) == key(b) != key(c) and len(set(key(a))) == 200
    pick = np.random.default_rng(3).permutation(len(rs))[:200]
    assert (a.row0 == rs.row0[pick]).all() and (a.path_ids == pick).all() and (a.hop_off == rs.hop_off[pick]).all()
    assert [it['path'] for it in a.items()] == [world['items'][i]['path'] for i in pick]
    assert len(rs.sample(len(rs), 1)) == len(rs)
    with pytest.raises(ValueError):
        rs.sample(len(rs) + 1, 1)


def test_an_env_over_the_written_split_walks_the_same_routes(world, tmp_path):
    from speaker_follower_amd import env as E, nav as N
    rs, nav = world['routes'].sample(120, 5), world['nav']
    path = str(tmp_path / 'R2R_aug.json')
    rs.write_split(path, first_path_id=1000)
    items = json.load(open(path))
    assert [it['path_id'] for it in items] == [1000 + int(p) for p in rs.path_ids] and items == rs.items(1000)
    e = E.R2RIndexEnv(items, world['env'].row_of, world['env'].nav_graph_path, batch_size=40, scans=nav.scans)
    table = N.NavTable(e, types.SimpleNamespace(device=torch.device('cpu')))
    n, rows = table.gold_routes(items, S)
    wn, wreached, wrows = rs.walk_host(S)
    assert (n == wn).all() and wreached.all()
    first = np.concatenate(([0], np.cumsum(n)))
    for i in range(len(items)):
        assert (rows[first[i]:first[i + 1], 0] == nav.host['feat_row'][wrows[:n[i], i]]).all()
        assert rows[first[i + 1] - 1, 5] == 1.0 and (rows[first[i]:first[i + 1] - 1, 5] == 0.0).all()


def mirror_blocks(nav, rs, B, Lmax):
    """The mirror's lengths mode, then its pack mode over blocks laid out as RouteSet.pack lays them out."""
    tab, hop = R.table_of(nav), nav.all_hops()
    args = (tab, S, rs.row0, rs.view0, rs.goal, hop, rs.hop_off, rs.hop_base, rs.hop_rows)
    first = R.mirror_routes(*args)
    N, M = len(rs), -(-len(rs) // B)
    route = (np.arange(M * B) % N).astype(np.int32)
    Tp, off, total = R.plan_blocks(first['n_actions'], route, B, Lmax)
    tokens = instr_off = None
    if rs.enc is not None:
        instr_off = np.concatenate(([0], np.cumsum([len(e) for e in rs.enc])))
        tokens = np.concatenate([np.asarray(e, np.int64) for e in rs.enc] + [np.zeros(0, np.int64)])
    packed = R.mirror_routes(*args, route=route, pack=dict(B=B, Lmax=Lmax, mb_Tp=Tp, mb_off=off, tokens=tokens,
                                                           instr_off=instr_off, out=np.full(total, 0x5A, np.uint8)))
    return first, packed, route, Tp, off


@pytest.mark.parametrize('B', [100, 7])
def test_the_mirror_writes_the_host_paths_bytes_for_every_enumerated_route(world, B):
    nav, rs = world['nav'], world['routes']
    first, packed, route, Tp, off = mirror_blocks(nav, rs, B, LMAX)
    wn, wreached, wrows = rs.walk_host(S)
    assert first['err'] == packed['err'] == 0 and (first['reached'] == 1).all()
    assert (first['n_actions'] == wn).all() and (first['rows'] == wrows).all()
    for k in ('n_actions', 'reached'):
        assert (packed[k] == first[k][route]).all()
    assert (packed['rows'] == first['rows'][:, route]).all()
    want = R.host_blocks(nav, world['items'], route, B, LMAX, S)
    assert [t for t, _ in want] == Tp.tolist()                        # the step count of every minibatch is the host path's
    for i, (t, buf) in enumerate(want):
        assert R.sections_equal(packed['out'][off[i]:off[i] + len(buf)], buf, B, t, LMAX) == [], i
    free = R.gap_mask(B, LMAX, Tp, off, len(packed['out']))
    assert (packed['out'][free] == 0x5A).all()                        # the gaps are not written


def test_from_items_on_the_fixture_split_and_at_every_instruction_length(world):
    from speaker_follower_amd.routes import RouteSet
    fx = json.load(open(os.path.join(HERE, 'golden', 'r2r_fixture_items.json')))['items']
    nav = world['nav']
    items = [dict(it, instr_encoding=np.asarray(it['instr_encoding'], np.int64)) for it in fx
             if (it['scan'], it['path'][0]) in nav.row_of]
    assert len(items) == len(fx) > 0
    rs = RouteSet.from_items(nav, items)
    rows, views = nav.start_states(items)
    assert (rs.row0 == rows).all() and (rs.view0 == views).all() and rs.instr_ids == [it['instr_id'] for it in items]
    assert [nav.vp_of[g][1] for g in rs.goal] == [it['path'][-1] for it in items] and rs.items() == items
    for B in (len(items), 4):
        first, packed, route, Tp, off = mirror_blocks(nav, rs, B, LMAX)
        for i, (t, buf) in enumerate(R.host_blocks(nav, items, route, B, LMAX, S)):
            assert t == Tp[i] and R.sections_equal(packed['out'][off[i]:off[i] + len(buf)], buf, B, t, LMAX) == [], (B, i)
    # instructions of 0, 1, Lmax - 2, Lmax - 1, Lmax and Lmax + 1 tokens (the last two lose their EOS)
    rng = np.random.default_rng(8)
    some = [dict(it, instr_encoding=rng.integers(4, 900, n).astype(np.int64), instr_id='%d_0' % i)
            for i, (it, n) in enumerate(zip(world['items'][::300], (0, 1, LMAX - 2, LMAX - 1, LMAX, LMAX + 1)))]
    assert len(some) == 6
    rs = RouteSet.from_items(nav, some)
    first, packed, route, Tp, off = mirror_blocks(nav, rs, 6, LMAX)
    (t, buf), = R.host_blocks(nav, some, route, 6, LMAX, S)
    assert R.sections_equal(packed['out'][:len(buf)], buf, 6, t, LMAX) == []
    seq = buf[:6 * LMAX * 8].view(np.int64).reshape(6, LMAX)
    assert (seq == R.EOS).sum(1).tolist() == [1, 1, 1, 1, 0, 0] and seq[5, -1] == some[5]['instr_encoding'][LMAX - 1]


def test_replaced_items_have_score_results_format(world):
    from speaker_follower_amd import speaker_evaluation
    rs = world['routes'].sample(30, 2)
    items = rs.items(first_path_id=7)
    results = {it['instr_id']: dict(instr_id=it['instr_id'], words=['w%d' % i, 'x', '<EOS>'][:1 + i % 3], score=-1.0 * i)
               for i, it in enumerate(items)}
    ev = speaker_evaluation.SpeakerEvaluation(items=items, instructions_per_path=1, device='cpu')
    got = rs.replaced_items(results, first_path_id=7)
    assert [g['path_id'] for g in got] == sorted(it['path_id'] for it in items)
    by_id = {it['path_id']: it for it in items}
    for g in got:
        want = dict(by_id[g['path_id']], instructions=[' '.join(results['%d_0' % g['path_id']]['words'])])
        assert g == want
    _, replaced = ev.score_results(results)
    assert replaced == got
