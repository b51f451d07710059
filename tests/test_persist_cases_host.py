"""CPU checks of tests/persist_cases.py: the float64 models against the oracle run end to end (torch_ref.speaker_score,
torch_ref.encoder_lstm / encoder_bilstm and their autograd), the case tables on both sides of every boundary the mirrored
constants define, and the comparator against seven corruptions of the model's own output -- what a persistent launch
with an off-by-one in its partition would hand back."""
import dataclasses

import numpy as np
import pytest
import torch

from oracle import torch_ref
from speaker_follower_amd import synth
from tests import persist_cases as PC

f64 = torch.float64
TINY = dataclasses.replace(synth.SMALL, hidden=16, vocab=23)


# ------------------------------------------------------------------------------- models vs the oracle
@pytest.mark.parametrize('vocab', [23, 33])                     # one small vocabulary, one at an edge of the slots
@pytest.mark.parametrize('feedback', ['teacher', 'argmax'])
def test_word_loop_model_agrees_with_the_oracle_end_to_end(vocab, feedback):
    dims = dataclasses.replace(TINY, vocab=vocab)
    enc_w, dec_w = synth.speaker_weights_peaky(7, dims)
    B, Tp, S, V, F = 5, 3, 6, 4, dims.feat
    rng = np.random.default_rng(vocab)
    acts = [rng.standard_normal((B, F)) for _ in range(Tp)]
    feats = [rng.standard_normal((B, V, F)) for _ in range(Tp)]
    mask = PC.path_mask(B, Tp)
    targets = PC.speaker_targets(rng, vocab, S, B)
    enc, dec = torch_ref.to_torch(enc_w, dtype=f64), torch_ref.to_torch(dec_w, dtype=f64)
    ref = torch_ref.speaker_score(enc, dec, acts, feats, torch.tensor(mask.astype(bool)), torch.tensor(targets.T.copy()), S,
                                  feedback)
    ctx, h0, c0 = torch_ref.speaker_encoder(enc, acts, feats)
    inp = PC.SpkInputs(ctx.numpy(), h0.numpy(), c0.numpy(), mask, targets)
    n = len(ref['logits'])                                       # (the oracle leaves its loop once every row has ended)
    words = np.concatenate((np.full((1, B), PC.BOS, np.int64), ref['words'].numpy()), 0)
    if feedback == 'argmax':
        assert np.array_equal(PC.argmax_rollout(dec_w, inp)[:n + 1], words)
    else:
        assert np.array_equal(words, PC.teacher_words(inp, B)[:n + 1])
    got = PC.word_loop(dec_w, PC.SpkInputs(*inp[:4], targets[:n]), words)
    np.testing.assert_allclose(got['logits'], torch.stack(ref['logits']).numpy(), rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(got['h1'][-1], ref['h'].numpy(), rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(got['c1'][-1], ref['c'].numpy(), rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(got['step_scores'].sum(0), ref['scores'].numpy(), rtol=1e-12, atol=1e-13)
    live = got['live'].astype(np.float64)
    loss = sum(got['nll_term'][t].sum() / live[t].sum() for t in range(n) if live[t].any())
    np.testing.assert_allclose(loss, float(ref['loss']), rtol=1e-12)
    assert np.array_equal(got['ended'], (words[1:] == PC.EOS).any(0).astype(np.uint8))
    mb = mask.astype(bool)
    assert not got['alpha'][:, mb].any() and np.abs(got['alpha'].sum(2) - 1).max() < 1e-14


@pytest.mark.parametrize('bidir', [False, True])
def test_encoder_model_agrees_with_the_oracle_and_its_autograd(bidir):
    w = synth.bidirectional_encoder_weights(5, TINY) if bidir else synth.follower_weights(5, TINY)[0]
    B, T = 6, 7
    seq, lens = PC.encoder_tokens(B, T, T + 2, seed=3, vocab=TINY.vocab)
    rng = np.random.default_rng(9)
    Hc = TINY.hidden
    drop = (rng.random((B, T * Hc)) < 0.5) * 2.0
    m = PC.encoder_model(w, seq, lens, drop_ctx=drop, grad=True)
    ref_w = torch_ref.to_torch(w, requires_grad=True, frozen=('embedding.weight',), dtype=f64)
    fn = torch_ref.encoder_bilstm if bidir else torch_ref.encoder_lstm
    ctx, h, c = fn(ref_w, torch.tensor(seq), lens, drop_ctx=torch.tensor(drop).reshape(B, T, Hc))
    for name, a, b in (('ctx', m['ctx'], ctx), ('decoder_init', m['decoder_init'], h), ('c_t', m['c_t'], c)):
        np.testing.assert_allclose(a.detach().numpy(), b.detach().numpy(), rtol=1e-12, atol=1e-14, err_msg=name)
    dctx, dh, dc = (torch.tensor(rng.standard_normal(tuple(x.shape))) for x in (ctx, h, c))
    ((m['ctx'] * dctx).sum() + (m['decoder_init'] * dh).sum() + (m['c_t'] * dc).sum()).backward()
    ((ctx * dctx).sum() + (h * dh).sum() + (c * dc).sum()).backward()
    for k, p in ref_w.items():
        if p.requires_grad:
            np.testing.assert_allclose(m['w'][k].grad.numpy(), p.grad.numpy(), rtol=1e-10, atol=1e-13, err_msg=k)
    # the retained gate gradients are the tape the launch writes: zero at dead steps, and their sum over steps and rows
    # is the bias gradient
    for d, sfx in (('f', ''), ('r', '_reverse'))[:2 if bidir else 1]:
        dg = torch.stack([p.grad for p in m[d]['pre']])
        for b, n in enumerate(lens):
            assert not dg[n:, b].any()
        np.testing.assert_allclose(dg.sum((0, 1)).numpy(), ref_w['lstm.bias_ih_l0' + sfx].grad.numpy(), rtol=1e-10, atol=1e-13)
    PC.check_ctx_beyond_lengths(m['ctx'].detach().numpy(), lens)
    PC.check_state_held(m['f']['hs'].detach().numpy(), m['f']['cs'].detach().numpy(), lens)


# --------------------------------------------------------------------------------- case-table coverage
def _values(table, field):
    return {getattr(c, field) for c in table}


def test_every_boundary_appears_on_both_sides():
    for name, table, field, below, above in PC.boundaries():
        vals = _values(table, field)
        assert below in vals, (name, 'below', below)
        if above is not None:
            assert above in vals, (name, 'above', above)
        elif table is PC.ENCODER:
            assert getattr(PC.ENCODER_FALLBACK, field) == below + 1 and not PC.encoder_supported(9, below + 1), name
        else:
            far = [getattr(r, field) for r in PC.REFUSALS if r.status == 2]
            assert (below + 1 in far) or (below - 1 in far), (name, 'no refusal one step past', below)
    for r in PC.REFUSALS:
        if r.status == 2:
            assert not PC.speaker_supported(r.B, r.Tp, r.vocab), r
    for c in PC.SPEAKER:
        assert PC.speaker_supported(c.B, c.Tp, c.vocab), c
    for c in PC.ENCODER + PC.ENCODER_BWD:
        assert PC.encoder_supported(c.B, c.T), c


def test_the_tables_reach_what_their_rows_are_there_for():
    vocabs, bs = _values(PC.SPEAKER, 'vocab'), _values(PC.SPEAKER, 'B')
    slots = {v: PC.vocab_slots(v) for v in vocabs}
    assert slots[935] == (29, 7, 2) and 991 in vocabs                        # the two live vocabularies
    half = PC.EP_SLOTS // 2
    assert any(full == 1 and part == 1 for full, part, _ in slots.values())              # a slot holding one column
    assert any(part == PC.VOC_COLS - 1 for _, part, _ in slots.values())
    assert any(full + bool(part) <= half - 1 for full, part, _ in slots.values())        # slots 15 AND 31 empty
    assert any(full == half and part == 0 for full, part, _ in slots.values())           # every second-half slot empty
    assert any(empty == 0 and part == 0 for _, part, empty in slots.values())
    rows = {b: PC.group_rows(b) for b in bs}
    assert all(sum(r) == b for b, r in rows.items())
    assert any(r.count(0) >= 1 and 1 in r for r in rows.values())            # empty groups beside a one-row group
    assert any(0 < r[-1] < PC.rpg(b) for b, r in rows.items())               # a ragged last group
    assert any(r == [PC.EP_ROWS] * PC.EP_GROUPS for r in rows.values())
    assert rows[1] == [1] + [0] * (PC.EP_GROUPS - 1)
    # every table row changes ONE dimension against the default (peaky rows: the weights as well)
    for c in PC.SPEAKER:
        diff = [k for k in ('vocab', 'Tp', 'B', 'S') if getattr(c, k) != PC.SPK_DEFAULT[k]]
        assert len(diff) <= 1, c
    for field, want in (('vocab', (33, 935, 1024)), ('Tp', (PC.SP_TPMAX,)), ('B', (PC.B_MAX - 7,))):
        assert set(want) <= {getattr(c, field) for c in PC.SPEAKER if c.peaky}
    assert {c.mask for c in PC.SPEAKER if c.Tp in PC.TPS} == {False, True}
    # ties: one thread's two columns, two lanes, neighbouring workgroups, slots s | s + 16 of one lane, the last column
    gaps = {(hi - lo) for v, (lo, hi) in PC.TIES if v == PC.VOCAB_MAX}
    assert gaps == {PC.VOC_COLS // 2, 1, PC.VOC_COLS, PC.VOC_COLS * half}
    for v, (lo, hi) in PC.TIES:
        assert lo < hi < v
        if hi - lo == PC.VOC_COLS // 2:
            assert lo // PC.VOC_COLS == hi // PC.VOC_COLS and lo % PC.VOC_COLS < PC.VOC_COLS // 2
        if hi - lo == 1:
            assert lo // PC.VOC_COLS == hi // PC.VOC_COLS
    v, (lo, hi) = PC.TIES[-1]
    assert hi == v - 1 and PC.vocab_slots(v)[1] and lo // PC.VOC_COLS < hi // PC.VOC_COLS
    assert {PC.vocab_slots(v)[2] > 0 for v in PC.SAMPLE_VOCABS} == {True, False}
    # the encoder's shapes: one step, the rotation's first turn, Lpad > T and Lpad == T, every length 1
    assert {c.T for c in PC.ENCODER} >= {1, 2, 3, 4, PC.EP_TMAX - 1, PC.EP_TMAX}
    assert any(c.Lpad > c.T for c in PC.ENCODER) and any(c.Lpad == c.T for c in PC.ENCODER)
    assert any(c.T == 1 and c.B > 1 for c in PC.ENCODER)
    assert {(c.B, c.T) for c in PC.ENCODER_BWD if not c.bidir} >= {(1, 1), (9, PC.EP_TMAX), (PC.B_MAX, 3)}
    assert [c.train for c in PC.ENCODER_BWD if not c.bidir] == [False, False, True, False, True]
    assert {(c.B, c.T) for c in PC.ENCODER_BWD if c.bidir} == {(1, 1), (9, PC.EP_TMAX)}


@pytest.mark.parametrize('case', [PC.SPEAKER[0], PC.SPEAKER[10], PC.SPEAKER[13], PC._spk(Tp=PC.SP_TPMAX), PC._spk(B=1, S=1)],
                         ids=lambda c: 'v%d-Tp%d-B%d-S%d' % c[:4])
def test_the_inputs_hold_the_rows_and_columns_the_edges_need(case):
    inp = PC.speaker_inputs(case)
    t = inp.targets
    assert t.shape == (case.S, case.B) and t.min() >= 0 and t.max() < case.vocab
    assert (t[:, 0] != PC.PAD).all()                                           # one row live at every step
    if case.B >= 3:
        assert (t[:, -1] == PC.PAD).all()                                      # one row all PAD
        live = (t != PC.PAD).sum(0)
        assert ((t != PC.PAD) == (np.arange(case.S)[:, None] < live[None, :])).all()      # PAD tails only
        for col in PC.special_columns(case.vocab) + [PC.PAD]:
            assert (t == col).any(), col
        assert PC.last_slot_first(case.vocab) in t and case.vocab - 1 in t
    m = PC.path_mask(case.B, case.Tp)
    lens = (m == 0).sum(1)
    assert lens[0] == case.Tp and (case.B < 2 or lens[1] == 1) and lens.min() >= 1
    assert ((m == 0) == (np.arange(case.Tp)[None, :] < lens[:, None])).all()
    assert float(np.abs(inp.ctx).max()) < 1 and float(np.abs(inp.h_init).max()) < 1
    seq, ln = PC.encoder_tokens(9, 5, 8)
    assert ln[0] == 5 and ln[-1] == 1 and all((seq[b, n:] == 0).all() and (seq[b, :n] >= 4).all() for b, n in enumerate(ln))
    assert PC.encoder_tokens(9, 1, 80)[1] == [1] * 9                           # every length 1


# ------------------------------------------------------------------------------------ mutation checks
MUT = PC._spk()                                   # vocab 935: 29 slots + 7 columns + 2 empty slots; B 9, Tp 3, S 4, ragged mask


@pytest.fixture(scope='module')
def families():
    """{'plain' | 'peaky': (decoder state, inputs, teacher words, float64 model, float32 model)}"""
    out = {}
    for name, peaky in (('plain', False), ('peaky', True)):
        dec = PC.speaker_decoder_weights(MUT.vocab, peaky)
        inp = PC.speaker_inputs(MUT)
        words = PC.teacher_words(inp, MUT.B)
        out[name] = (dec, inp, words, PC.word_loop(dec, inp, words), PC.word_loop(dec, inp, words, torch.float32))
    return out


def _rejected_by(families, corrupt, keys=('logits',), check=None):
    """The families whose comparator refuses corrupt(family) -> a model output; at least one must."""
    hit = []
    for name, fam in families.items():
        bad = corrupt(*fam)
        print('%s: logits moved by %.2e of their scale' % (name, PC.rel_err(bad['logits'], fam[3]['logits'])))
        try:
            if check is not None:
                check(bad, fam)
            else:
                PC.compare(name, bad, fam[3], fam[4], keys)
        except AssertionError:
            hit.append(name)
    assert hit, 'accepted with the plain AND the peaky weights'
    return hit


def test_the_reference_itself_passes_and_stays_below_the_ceiling(families):
    for name, (dec, inp, words, r64, r32) in families.items():
        rows = []
        PC.compare(name + ' float32 model', r32, r64, r32, PC.TENSORS, rows=rows)
        for _, k, e, e32, b in rows:
            assert PC.K * e32 < PC.CEILING and b < PC.CEILING, (k, e32)
        assert np.array_equal(PC.argmax_rollout(dec, inp, torch.float32), PC.argmax_rollout(dec, inp))
        PC.check_exact_flags(r32, r64, words)
        PC.check_alpha(r32['alpha'], inp.mask)


def test_mutation_attention_scores_without_one_slot(families):
    """(1) one workgroup's 16 units left out of the attention scores: s_l = sum_j cq[l, j] h1[j] without j in a slot."""
    def corrupt(dec, inp, words, r64, r32):
        w_in = dec['attention_layer.linear_in.weight'].copy()
        w_in[:, 5 * PC.SLOT_UNITS:6 * PC.SLOT_UNITS] = 0                        # target = W_in h1 never sees those units
        return PC.word_loop(dict(dec, **{'attention_layer.linear_in.weight': w_in}), inp, words)
    _rejected_by(families, corrupt, ('logits',))
    _rejected_by(families, corrupt, ('alpha',))


def test_mutation_path_mask_ignored_for_one_row(families):
    """(2)"""
    def corrupt(dec, inp, words, r64, r32):
        m = inp.mask.copy()
        m[1] = 0
        return PC.word_loop(dec, inp, words, mask=m)
    _rejected_by(families, corrupt, ('logits',))
    assert len(_rejected_by(families, corrupt, check=lambda bad, fam: PC.check_alpha(bad['alpha'], fam[1].mask))) == 2


def test_mutation_last_slot_left_out_of_the_log_sum_exp(families):
    """(3) must show in step_scores and in nll_term, each on its own."""
    def corrupt(dec, inp, words, r64, r32):
        bad = PC.word_loop(dec, inp, words, lse_cols=PC.last_slot_first(MUT.vocab))
        assert np.array_equal(bad['logits'], r64['logits'])
        return bad
    _rejected_by(families, corrupt, ('step_scores',))
    _rejected_by(families, corrupt, ('nll_term',))


def test_mutation_last_column_reads_its_neighbour(families):
    """(4) the clamped weight-row load min(col, vocab - 1) without its `col < vocab` guards, seen from the other side: the
    logit of column vocab - 1 replaced by that of column vocab - 2."""
    def corrupt(dec, inp, words, r64, r32):
        bad = dict(r64, logits=r64['logits'].copy())
        bad['logits'][..., -1] = bad['logits'][..., -2]
        return bad
    _rejected_by(families, corrupt, ('logits',))


def test_mutation_tie_resolved_to_the_higher_index(families):
    """(5)"""
    for vocab, pair in PC.TIES:
        good = np.full((PC.TIE_S + 1, PC.TIE_B), pair[0], np.int64)
        PC.check_tie_words(good, pair)
        bad = good.copy()
        bad[2, 3] = pair[1]
        with pytest.raises(AssertionError):
            PC.check_tie_words(bad, pair)
    # and the argmax rule: the word one place below the float64 maximum is refused, the arg max accepted
    for dec, inp, words, r64, r32 in families.values():
        b_abs = PC.logit_bound_abs(r64, r32)
        best = np.concatenate((words[:1], r64['logits'].argmax(2)), 0)
        PC.check_argmax_words(best, r64['logits'], b_abs)
        second = best.copy()
        second[1:] = np.argsort(r64['logits'], axis=2)[:, :, -2]
        with pytest.raises(AssertionError):
            PC.check_argmax_words(second, r64['logits'], b_abs)


@pytest.fixture(scope='module')
def encoder_family():
    w = synth.follower_weights(101)[0]
    seq, lens = PC.encoder_tokens(9, 6, 80)
    m64 = PC.encoder_model(w, seq, lens)
    m32 = PC.encoder_model(w, seq, lens, dtype=torch.float32)
    flat = lambda m: dict(hs=m['f']['hs'].double().numpy(), cs=m['f']['cs'].double().numpy(),        # noqa: E731
                          gates=m['f']['gates'].double().numpy(), ctx=m['ctx'].double().numpy())
    return w, seq, lens, flat(m64), flat(m32), flat


def test_mutation_ctx_beyond_a_length_not_zero(encoder_family):
    """(6)"""
    w, seq, lens, r64, r32, flat = encoder_family
    PC.check_ctx_beyond_lengths(r64['ctx'], lens)
    PC.check_state_held(r64['hs'], r64['cs'], lens)
    bad = r64['ctx'].copy()
    bad[-1, lens[-1], 7] = 1e-30
    with pytest.raises(AssertionError):
        PC.check_ctx_beyond_lengths(bad, lens)
    hs = r64['hs'].copy()
    hs[-1, -1, 0] = np.nextafter(hs[-1, -1, 0], 1.0)
    with pytest.raises(AssertionError):
        PC.check_state_held(hs, r64['cs'], lens)


def test_mutation_encoder_step_reads_the_next_token(encoder_family):
    """(7)"""
    w, seq, lens, r64, r32, flat = encoder_family
    PC.compare('float32 encoder', r32, r64, r32, ('hs', 'cs', 'gates', 'ctx'))
    bad = flat(PC.encoder_model(w, seq, lens, shift=1))
    for k in ('hs', 'gates', 'ctx'):
        with pytest.raises(AssertionError):
            PC.compare('mutation 7', bad, r64, r32, (k,))
