"""CPU: the case builders, the float32 order models and the rule of tests/speaker_sample_cases.py, and the two edges of
the draw's contract in the float64 mirror (oracle/rng.py::speaker_sample): an empty slot is never drawn, the level-2
fallback is the last column that carries weight.  No GPU."""
import numpy as np
import pytest

from oracle import rng as orng
from tests import choice_models as CM
from tests import speaker_sample_cases as SC

F32 = np.float32


# ---- the recorded edge rows --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('special', SC.SPECIALS)
def test_every_recorded_edge_row_has_its_uniform(special):
    where, which, value, _ = SC.EDGES[special]
    assert where['seed'] == SC.SEED
    u = orng.sample_uniforms(where['seed'], where['stream'], [where['row']])[which][0]
    assert u == value                                                   # exactly: 0, (2^24 - 1) / 2^24, 0.5
    assert SC.U_ONE == (2 ** 24 - 1) / 2 ** 24


@pytest.mark.parametrize('vocab,special', [(v, s) for v, s, _ in SC.GLUE_CASES if s])
def test_the_special_row_of_a_launch_meets_its_edge_uniform(vocab, special):
    case = SC.speaker_sample_case(vocab, special)
    ex = SC.case_expectation(vocab, special)
    _, which, value, _ = SC.EDGES[special]
    assert (ex['u1'], ex['u2'])[which][case['at']] == value
    assert case['kind'][case['at']] == special


@pytest.mark.parametrize('vocab', SC.PERSIST_VOCABS)
def test_the_special_launches_of_the_word_loop_meet_their_edge_at_a_later_step(vocab):
    for name, row, stream, row0, info in SC.persist_rows(vocab):
        if name in SC.EDGES:
            _, which, value, _ = SC.EDGES[name]
            assert stream >= 0 and SC.P_T > 0
            assert SC.persist_uniforms(stream, row0)[which][SC.P_T * SC.P_B + SC.P_ROW] == value


# ---- the cap: a condition on the inputs, asserted on the mirror alone ---------------------------------------------------
@pytest.mark.parametrize('vocab,special,seed', SC.GLUE_CASES)
def test_every_glue_case_keeps_a_clear_share_of_at_least_099(vocab, special, seed):
    ex = SC.case_expectation(vocab, special, seed)
    assert ex['clear'].mean() >= 0.99, (vocab, special, seed, ex['clear'].mean())
    # the mirror itself satisfies the rule
    case = SC.speaker_sample_case(vocab, special, seed)
    assert SC.check_draws('mirror', ex['w'], case['logit'], ex)['share'] >= 0.99


@pytest.mark.parametrize('vocab', SC.PERSIST_VOCABS)
@pytest.mark.parametrize('finite_only', (False, True))
def test_the_word_loop_launches_of_a_vocabulary_keep_a_clear_share_of_at_least_099(vocab, finite_only):
    n = len(SC.persist_rows(vocab, finite_only))
    clear = np.concatenate([SC.persist_expectation(vocab, i, finite_only)['clear'] for i in range(n)])
    assert clear.mean() >= 0.99, (vocab, n, clear.mean())


def test_the_launches_hold_every_row_kind_and_every_dead_pattern():
    for vocab in SC.GLUE_VOCABS:
        case = SC.speaker_sample_case(vocab)
        x, kind = case['logit'], case['kind']
        assert set(kind) == set(SC.KINDS)
        ns = SC.n_slots(vocab)
        seg = np.full((SC.B, ns * 32), -np.inf, F32)
        seg[:, :vocab] = x
        seg = seg.reshape(SC.B, ns, 32)
        top = seg.max(2)
        empty = np.isneginf(top).sum(1)
        assert (empty[kind == 'empty1'] == 1).all() and (empty[kind == 'empty_all_but_one'] == ns - 1).all()
        assert (empty[kind == 'one_column'] == ns - 1).all() and (np.isfinite(x[kind == 'one_column']).sum(1) == 1).all()
        assert set(empty[kind == 'empty2']) == {min(2, ns - 1)}
        e1 = np.isneginf(top[kind == 'empty1'])
        assert e1[:, 0].any() and e1[:, ns - 1].any()                    # slot 0 and the ragged last slot among them
        for k, how in (('tail5', 'under'), ('tail5_inf', 'inf'), ('head16', 'under'), ('head1_inf', 'inf')):
            rows = np.flatnonzero(kind == k)
            with np.errstate(invalid='ignore'):
                d = seg[rows] - top[rows][:, :, None]
            dead = np.isneginf(d) if how == 'inf' else (d < -SC.UNDERFLOW - 1) & np.isfinite(d)
            assert dead.any(2).any(1).mean() >= 0.6, (vocab, k)       # (a ragged last slot of one column has no tail)
        assert (np.abs(x[kind == 'shift+80'].max(1) - 80) < 20).all() and (np.abs(x[kind == 'shift-80'].max(1) + 80) < 20).all()
        ex = SC.case_expectation(vocab)
        assert (ex['w'][kind == 'last_slot'] >= 32 * (ns - 1)).mean() > 0.5           # the mass sits in the last slot
        if vocab > 1024:                                                             # the carry across panels is used
            assert (ex['w'] >= 1024).mean() > {1025: 0.0, 1086: 0.03, 4096: 0.4}[vocab]


# ---- the contract's two edges in the mirror -----------------------------------------------------------------------------
def test_the_mirror_never_draws_an_empty_slot_over_a_sweep_of_u1():
    rng = np.random.default_rng(11)
    sweep = np.concatenate([[0.0, SC.U_ONE, 0.5], np.arange(0, 2 ** 24, 2 ** 24 // 509) / 2.0 ** 24])
    n = 0
    for vocab in (37, 991, 1086):
        ns = SC.n_slots(vocab)
        for kind in ('empty1', 'empty2', 'empty_all_but_one', 'one_column'):
            for i in range(3):
                row = SC.build_row(vocab, kind, rng, 3 * i)
                empty = {s for s in range(ns) if not np.isfinite(row[32 * s:32 * s + 32]).any()}
                assert empty
                for u1 in sweep:
                    for und in (None, SC.UNDERFLOW):
                        w, margin, d = orng.speaker_sample(row, u1, 0.37, underflow=und, detail=True)
                        assert d['slot'] not in empty and np.isfinite(row[w]) and np.isfinite(margin)
                        assert np.isfinite(d['p']).all() and (d['p'][sorted(empty)] == 0).all()
                        n += 1
    assert n > 10000
    with pytest.raises(AssertionError, match='outside the contract'):
        orng.speaker_sample(np.full(40, -np.inf), 0.5, 0.5)


def test_the_mirrors_level_2_fallback_is_the_last_column_that_carries_weight():
    """The fallback is reached when u2 * z_s >= every prefix: u2 >= 1 (the corner above U_ONE)."""
    rng = np.random.default_rng(12)
    for vocab in (37, 1024):
        for kind in ('tail1', 'tail5', 'tail16', 'tail1_inf', 'tail5_inf', 'tail16_inf', 'one_column', 'plain'):
            for i in range(6):
                row = SC.build_row(vocab, kind, rng, i)
                for u1 in (0.0, 0.3, SC.U_ONE):
                    w, _, d = SC.mirror(row, u1, SC.U_ONE * (1 + SC.CORNER))
                    assert d['fallback2'] and d['e'][d['col']] > 0 and not (d['e'][d['col'] + 1:] > 0).any()
                    s = d['slot']
                    assert row[w] >= row[32 * s:32 * s + 32].max() - SC.UNDERFLOW
                    # without the keyword every float64 weight counts: -inf columns still never
                    w64 = orng.speaker_sample(row, u1, 1.0)[0]
                    assert np.isfinite(row[w64])
    # the pair (word, margin) of the older callers is unchanged on ordinary rows
    row = (rng.standard_normal(991) * 1.5).astype(F32)
    for u1, u2 in rng.random((50, 2)):
        w, m = orng.speaker_sample(row, u1, u2)
        p = CM.softmax64(row)
        assert w == int(np.flatnonzero(np.cumsum(p) > _inverse(p, u1, u2))[0]) or m < 1e-9


def _inverse(p, u1, u2):
    """The two-level draw as ONE threshold on the flat cdf: the slot's lower edge + u2 * its mass."""
    ns = -(-len(p) // 32)
    ps = np.array([p[32 * s:32 * s + 32].sum() for s in range(ns)])
    c = np.cumsum(ps)
    s = int(np.flatnonzero(c > u1 * c[-1])[0])
    return (c[s] - ps[s]) + u2 * ps[s]


# ---- the float32 order models ------------------------------------------------------------------------------------------
def test_the_order_models_sum_exactly_where_float32_is_exact():
    e = np.zeros(32, F32)
    e[[7, 23]] = 1
    for sums in (SC.f32_slot_sums, SC.f32_row16_sums):
        cum, tot = sums(e)
        assert tot == 2 and np.array_equal(cum, np.cumsum(e))
        assert SC.predicted_pick(e, 0.5, sums) == 23 and SC.predicted_pick(e, 0.0, sums) == 7
    e = np.arange(1, 33).astype(F32)                                     # small integers: every order gives the same sums
    for sums in (SC.f32_slot_sums, SC.f32_row16_sums):
        cum, tot = sums(e)
        assert np.array_equal(cum, np.cumsum(e)) and tot == e.sum()
    cdf, Z = SC.f32_level1_glue(np.ones(31, F32))
    assert np.array_equal(cdf[:31], np.arange(1, 32)) and Z == 31


def test_the_order_models_do_predict_a_miss_for_the_u2_one_rows_they_built():
    rows = [(v, s) for v in SC.GLUE_VOCABS + SC.PERSIST_VOCABS for s in ('u2_one', 'u2_one_inf')]
    for vocab, special in rows:
        if vocab in SC.GLUE_VOCABS:
            case = SC.speaker_sample_case(vocab, special)
            row, info = case['logit'][case['at']], case['info']
        else:
            row, info = next((r, i) for n, r, _, _, i in SC.persist_rows(vocab) if n == special)
        assert info['miss_glue'] and info['miss_persist'], (vocab, special, info)
        s = info['slot']
        seg = row[32 * s:32 * s + 32]
        e = SC.f32_weights(seg)
        assert (e[-5:] == 0).all() and (e[:-5] > 0).all()
        for sums in (SC.f32_slot_sums, SC.f32_row16_sums):
            assert SC.predicted_pick(e, SC.U_ONE, sums) is None
        # the mirror takes the last column that carries weight there, through the hit (u2 z_s < z_s in float64)
        w, margin, d = SC.mirror(row, 0.5, SC.U_ONE)
        assert d['slot'] == s and w == 32 * s + 26 and margin < SC.CLEAR
    # how often an ordinary slot misses at U_ONE under each order (the rate the issue's simulation reports for the glue)
    rng = np.random.default_rng(3)
    for sums, lo in ((SC.f32_slot_sums, 0.1), (SC.f32_row16_sums, 0.02)):
        miss = np.mean([SC.predicted_pick(SC.f32_weights((rng.standard_normal(32) * 1.5).astype(F32)), SC.U_ONE, sums) is None
                        for _ in range(1000)])
        print('%s: no column passes at U_ONE in %.3f of 1000 random slots' % (sums.__name__, miss))
        assert miss > lo


def test_the_level_1_order_models_sum_exactly_where_float32_is_exact():
    p = np.arange(1, 101).astype(F32)                                    # small integers, 4 panels: the carry is the prefix
    cdf, Z = SC.f32_level1_wide(p)
    assert np.array_equal(cdf, np.cumsum(p)) and Z == p.sum()
    m = np.zeros(30, F32)
    z = np.arange(1, 31).astype(F32)                                     # equal maxima: every wexp is 1, Z the plain sum
    cdf, Z, w = SC.f32_level1_persist(m, z)
    assert np.array_equal(w[:30], z) and np.array_equal(cdf[:30], np.cumsum(z)) and Z == z.sum()
    m[3] = -np.inf                                                       # an empty slot: weight 0, nothing is NaN
    cdf, Z, w = SC.f32_level1_persist(m, z)
    assert w[3] == 0 and Z == z.sum() - 4 and np.isfinite(cdf).all()


def test_the_order_models_do_predict_a_level_1_miss_for_the_u1_one_rows_they_built():
    """Every kernel that takes the row falls back to the arg max's slot under its own model: speaker_sample_row and the
    word loop up to 1024 words, the wide kernel above.  With one live slot (37 and 33 words) there is nothing to miss."""
    for vocab in SC.GLUE_VOCABS:
        case = SC.speaker_sample_case(vocab, 'u1_one')
        row, info = case['logit'][case['at']], case['info']
        want = {37: (), 991: ('glue', 'persist'), 1024: ('glue', 'persist')}.get(vocab, ('wide',))
        assert tuple(sorted(info['miss1'])) == tuple(sorted(want)) and all(info['miss1'].values()), (vocab, info)
        for o in want:
            assert SC.level1_misses(row, o)
        ex = SC.case_expectation(vocab, 'u1_one')
        assert not ex['clear'][case['at']] and (not want or len(ex['allowed'][case['at']]) == 2)
        assert int(np.argmax(row)) < 32 and (not want or ex['w'][case['at']] >= 32)       # mirror: the last live slot; fallback: slot 0
    for vocab in SC.PERSIST_VOCABS:
        for name, row, _, _, info in SC.persist_rows(vocab):
            if name == 'u1_one':
                want = () if vocab == 33 else ('glue', 'persist')
                assert tuple(sorted(info['miss1'])) == want and all(info['miss1'].values()), (vocab, info)
                for o in want:
                    assert SC.level1_misses(row, o)
    # an ordinary row misses under each order now and then, not always
    rng = np.random.default_rng(4)
    for order, vocab in (('glue', 991), ('persist', 991), ('wide', 4000)):   # (not 4096: a last live slot in lane 62 never misses)
        miss = np.mean([SC.level1_misses((rng.standard_normal(vocab) * 1.5).astype(F32), order) for _ in range(60)])
        print('%s: no slot passes at U_ONE in %.2f of 60 random rows' % (order, miss))
        assert 0 < miss < 1


# ---- the rule ---------------------------------------------------------------------------------------------------------------
def test_the_rule_refuses_what_it_is_there_to_refuse():
    vocab = 991
    case = SC.speaker_sample_case(vocab, 'u2_one')
    ex = SC.case_expectation(vocab, 'u2_one')
    x, at = case['logit'], case['at']
    good = ex['w'].copy()
    assert SC.check_draws('ok', good, x, ex)['share'] >= 0.99
    s = case['info']['slot']

    def refused(w, match):
        with pytest.raises(AssertionError, match=match):
            SC.check_draws('t', w, x, ex)
    w = good.copy()
    w[at] = 32 * s + 31                                                  # the old fallback: the slot's last column, dead
    refused(w, 'exactly 0')
    case_inf = SC.speaker_sample_case(vocab, 'u2_one_inf')
    w = SC.case_expectation(vocab, 'u2_one_inf')['w'].copy()
    w[at] = 32 * s + 31
    with pytest.raises(AssertionError, match='whose logit is -inf'):
        SC.check_draws('t', w, case_inf['logit'], SC.case_expectation(vocab, 'u2_one_inf'))
    w = good.copy()
    w[3] = vocab
    refused(w, 'outside')
    i = int(np.flatnonzero(case['kind'] == 'empty1')[0])
    w = good.copy()
    gone = int(np.flatnonzero(~np.isfinite(x[i]))[0])
    w[i] = gone
    refused(w, 'no finite column')
    i = int(np.flatnonzero(ex['clear'])[5])
    w = good.copy()
    w[i] = good[i] + 1 if good[i] + 1 < vocab and np.isfinite(x[i, good[i] + 1]) and x[i, good[i] + 1] > x[i, good[i]] - 50 else good[i] - 1
    refused(w, 'clear rows differ')
    # an unclear row: only the mirror's words at the corners
    assert not ex['clear'][at] and good[at] in ex['allowed'][at]
    w = good.copy()
    w[at] = good[at] - 1
    refused(w, 'unclear row')
    # the rows that are exact in float32 must take the mirror's word although their margin is 0
    for sp, other in (('u2_half', 32 * SC.fixed_slot(vocab) + 7), ('u1_half', 5)):
        c, e = SC.speaker_sample_case(vocab, sp), SC.case_expectation(vocab, sp)
        assert e['exact'][at] and not e['clear'][at] and e['margin'][at] == 0
        assert other in e['allowed'][at] and e['w'][at] != other          # `>=` would draw `other`
        w = e['w'].copy()
        w[at] = other
        with pytest.raises(AssertionError, match='clear rows differ'):
            SC.check_draws('t', w, c['logit'], e)
    # u = 0: the first item that carries weight, clear
    for sp in ('u1_zero', 'u2_zero', 'u2_zero_inf'):
        c, e = SC.speaker_sample_case(vocab, sp), SC.case_expectation(vocab, sp)
        assert e['clear'][at]
        row = c['logit'][at]
        if sp == 'u1_zero':
            assert e['slot'][at] == 2 and np.isneginf(row[:64]).all()
        else:
            s0 = 32 * SC.fixed_slot(vocab)
            assert e['w'][at] == s0 + (16 if sp == 'u2_zero' else 1)
    c, e = SC.speaker_sample_case(vocab, 'u1_one'), SC.case_expectation(vocab, 'u1_one')
    ns = SC.n_slots(vocab)
    assert e['slot'][at] == ns - 3 and not e['clear'][at]                # the last slot that carries weight; the corner
    assert any(a < 32 for a in e['allowed'][at])                         # above allows the arg max's slot, slot 0
    assert c['info']['miss_glue']
