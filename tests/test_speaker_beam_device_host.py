"""CPU: the host side of the speaker's device beam search (search.DeviceSpeakerBeam / sf_speaker_beam_select).

* frontier.speaker_beam_outputs -- the result assembly the host and device word loops share -- gives what the host
  loop's own tail gave before it was factored out, on synthetic hypotheses with exact score ties;
* the device loop's history layout (include/sf_hip.h: sf_speaker_beam_select), produced by a launch-by-launch numpy
  model of the kernel (`model_step`, which tests/test_gpu_choice_kernels.py holds the kernel to bit for bit) and read
  back through search.speaker_beam_nodes, gives the host loop's results (frontier.speaker_beam_search over a stand-in
  decoder whose log-probabilities are a function of the word history, with many ties);
* `model_step` gives what the one-function model it was taken out of gave, and the constructed inputs of the
  kernel-alone test reach every case that test is there for (ties, EOS at once, a full completion list, short lists);
* the new C entry rejects bad arguments before touching the device."""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

F32 = np.float32
BOS, EOS = 3, 2                  # speaker_follower_amd.follower (utils.py:19-24)


class Tok:
    def decode_sentence(self, encoding, break_on_eos=False, join=True):
        out = []
        for ix in encoding:
            if ix == (EOS if break_on_eos else 0):
                break
            out.append(str(int(ix)))
        return ' '.join(out) if join else out


def reference_tail(start_obs, perm, done, P, W, S, R, beam_size, attention_rows, tok):
    """frontier.speaker_beam_search's result assembly as it stood before it was shared (verbatim)."""
    B = len(start_obs)
    outputs = [[] for _ in range(B)]
    for b, src in enumerate(perm):
        assert not outputs[src]
        lst = done[b]
        for i in np.lexsort((np.arange(len(lst)), -S[lst]))[:beam_size]:
            lin = []
            n = lst[i]
            while n >= 0:
                lin.append(n)
                n = P[n]
            lin = lin[::-1]                              # BOS root first
            sc = [float(S[n]) for n in lin]
            words = [int(W[n]) for n in lin[1:]]
            outputs[src].append({
                'instr_id': start_obs[b]['instr_id'], 'word_indices': words, 'score': sc[-1],
                'scores': [y - x for x, y in zip(sc, sc[1:])],
                'words': tok.decode_sentence(words, break_on_eos=True, join=False) if tok is not None else list(words),
                'attentions': attention_rows([int(R[n]) for n in lin[1:]])})
    return outputs


def assert_same(got, want):
    assert len(got) == len(want)
    for gl, wl in zip(got, want):
        assert len(gl) == len(wl)
        for g, w in zip(gl, wl):
            assert set(g) == set(w)
            for key in ('instr_id', 'word_indices', 'score', 'scores', 'words'):
                assert g[key] == w[key], key
            assert len(g['attentions']) == len(w['attentions'])
            for a, b in zip(g['attentions'], w['attentions']):
                assert a.dtype == b.dtype and np.array_equal(a, b)


def test_shared_assembly_matches_the_host_tail_with_ties():
    from speaker_follower_amd import frontier
    rng = np.random.default_rng(3)
    B, beam, Tp = 5, 4, 3
    # a random forest of hypotheses: roots 0..B-1, every later node a child of an earlier node of the same instance
    P, I = [-1] * B, list(range(B))
    for n in range(B, 200):
        p = int(rng.integers(0, n))
        P.append(p)
        I.append(I[p])
    P, I = np.array(P), np.array(I)
    W = np.where(P < 0, BOS, rng.integers(0, 9, len(P)))
    S = np.zeros(len(P), F32)
    for n in range(B, len(P)):
        S[n] = F32(S[P[n]] + F32(-0.5 * rng.integers(0, 3)))       # coarse steps: many exact ties
    R = rng.permutation(len(P))
    att = rng.random((len(P), Tp)).astype(F32)
    done = [[int(n) for n in rng.permutation(np.flatnonzero((I == b) & (P >= 0)))[:7]] for b in range(B)]
    assert any(len(set(S[d].tolist())) < len(d) for d in done)
    start_obs = [{'instr_id': 'i%d' % b} for b in range(B)]
    perm = list(rng.permutation(B))
    rows = lambda r: list(att[r]) if r else []                      # noqa: E731
    for tok in (Tok(), None):
        want = reference_tail(start_obs, perm, done, P, W, S, R, beam, rows, tok)
        got = frontier.speaker_beam_outputs(start_obs, perm, done, P, W, S, R, beam, rows, tok)
        assert_same(got, want)


# ---- a stand-in decoder: top-k of log-probabilities that are a function of the word history (ties included)
VOCAB, TP = 9, 3


def lineage_logp(lineage):
    rng = np.random.default_rng(zlib.crc32(np.asarray(lineage, np.int64).tobytes()))
    lp = (-0.5 * rng.integers(0, 6, VOCAB)).astype(F32)
    lp[EOS] = F32(-0.5 * (5 - min(len(lineage), 5)))                # EOS more likely as the history grows
    return lp


def lineage_alpha(lineage):
    rng = np.random.default_rng(zlib.crc32(np.asarray(lineage, np.int64).tobytes()) ^ 0x5bd1)
    return rng.random(TP).astype(F32)


def topk(lp, k):
    o = np.lexsort((np.arange(len(lp)), -lp))[:k]                    # descending, ties: lower column first
    return o, lp[o]


class FakeFlatDecoder:
    """search.FlatSpeakerDecoder's interface over lineage_logp: pool row -> word history of the state."""

    def __init__(self, decoder, ctx, path_mask, pad_rows=None):
        self.hist = {}
        self.att = {}

    def seed(self, h, c):
        for b in range(h.shape[0]):
            self.hist[b] = (b,)
        self.n = h.shape[0]

    def step(self, words, rows, inst, k):
        base = self.n
        k = min(k, VOCAB)
        tw, tl = np.zeros((len(words), k), np.int64), np.zeros((len(words), k), F32)
        for i, (w, r) in enumerate(zip(words, rows)):
            lin = self.hist[int(r)] + (int(w),)
            self.hist[base + i] = lin
            self.att[base + i] = lineage_alpha(lin)
            tw[i], tl[i] = topk(lineage_logp(lin), k)
        self.n += len(words)
        return base, tw, tl

    def attention_rows(self, rows):
        return [self.att[r].copy() for r in rows]


class FakeSpeaker:
    def __init__(self, B, T):
        self.B, self.instruction_len, self.decoder = B, T, None
        self.env = type('E', (), {'tokenizer': Tok()})()
        self.encoder = lambda acts, feats: (torch.zeros(B, TP, 4), torch.zeros(B, 4), torch.zeros(B, 4))

    def _batch_observations_and_actions(self, path_obs, path_actions, enc):
        return ([{'instr_id': 'p%d' % b} for b in range(self.B)], None, None, torch.zeros(self.B, TP), None, None,
                list(range(self.B)))


# ------------------------------------------------------------------------------------------ the kernel's model
POISON = 0x7fc0dead              # an int32 pattern (a NaN as float32) for places the contract does not name


def new_state(B, beam, T, Tp, eos=EOS, bos=BOS, with_attn=True, ld=None):
    """The buffers of sf_spk_beam as DeviceSpeakerBeam presets them; every history array is [T, ld_hist] (ld_hist
    defaults to the smallest the entry accepts) and filled with POISON, as are the completion lists."""
    R = B * beam
    ld = (R * Tp if with_attn else R) if ld is None else ld
    poison = lambda *shape: np.full(shape, POISON, np.int32)                    # noqa: E731
    s = dict(B=B, beam=beam, T=T, Tp=Tp, eos=eos, ld=ld,
             score=np.zeros(R, F32), words=np.full(R, eos, np.int64), parent=np.full(R, -1, np.int32),
             inst=np.zeros((B, 3), np.int32), live_total=np.zeros(T, np.int32),
             hist_word=poison(T, ld), hist_parent=poison(T, ld), hist_score=poison(T, ld).view(F32),
             hist_attn=poison(T, ld).view(F32) if with_attn else None,
             done_rec=poison(B, 2 * beam), done_score=poison(B, 2 * beam).view(F32))
    s['words'][::beam] = bos
    s['parent'][::beam] = np.arange(0, R, beam)
    s['inst'][:, 0] = 1
    return s


def model_step(s, top_w, top_lp, alpha, trace=None):
    """One launch of sf_speaker_beam_select (include/sf_hip.h) on the buffers `s`, in place.  top_w int32 / top_lp
    float32 [R, k] as sf_logprob_topk gives them; alpha [R, Tp], or None when the state keeps no attention history.
    Returns [(b, successors)] of the instances that moved: the selections (score, flat index, slot i inside the
    instance, word) that became the next step's slots base, base + 1, ..  trace (optional dict of counters): which
    cases of the contract this launch went through."""
    B, W, T, Tp, eos = s['B'], s['beam'], s['T'], s['Tp'], s['eos']
    R, k = B * W, top_w.shape[1]
    tr = trace if trace is not None else {}
    bump = lambda name, n=1: tr.__setitem__(name, tr.get(name, 0) + n)          # noqa: E731
    moved = []
    for b in range(B):
        live, n_done, t = (int(x) for x in s['inst'][b])
        if live <= 0 or t >= T:
            bump('noop')                                     # an ended instance: the launch changes nothing
            continue
        base = b * W
        sc = (s['score'][base:base + live, None] + top_lp[base:base + live]).astype(F32).ravel()    # one float32 add
        order = np.lexsort((np.arange(live * k), -sc.astype(np.float64)))      # score descending, then flat index i*k + j
        cands = [(sc[n], int(n), int(n) // k, int(top_w[base + n // k, n % k])) for n in order[:W + 1]]
        sel = cands[:W]
        fin = [c[3] == eos or t == T - 1 for c in sel]
        cont = [c for c, f in zip(sel, fin) if not f]
        finals = [c for c, f in zip(sel, fin) if f]
        for p, c in enumerate(cont + finals):
            s['hist_word'][t, base + p], s['hist_parent'][t, base + p], s['hist_score'][t, base + p] = c[3], base + c[2], c[0]
        for q, c in enumerate(finals):
            s['done_rec'][b, n_done + q] = t * R + base + len(cont) + q
            s['done_score'][b, n_done + q] = c[0]
        if s['hist_attn'] is not None:                       # alpha[i] of the GLOBAL slot i = base + its place
            s['hist_attn'][t, base * Tp:(base + live) * Tp] = np.asarray(alpha, F32)[base:base + live].ravel()
        done_after = n_done + len(finals)
        live_next = 0 if done_after >= W else len(cont)
        moved.append((b, cont[:live_next]))
        for p, c in enumerate(cont[:live_next]):
            s['words'][base + p], s['parent'][base + p], s['score'][base + p] = c[3], base + c[2], c[0]
        s['words'][base + live_next:base + W] = eos
        s['parent'][base + live_next:base + W] = -1
        s['score'][base + live_next:base + W] = 0
        s['inst'][b] = live_next, done_after, t + 1
        s['live_total'][t] += live_next
        # ---- which cases this was
        for x, y in zip(cands, cands[1:len(sel) + 1]):       # neighbours in the order, the first one selected
            if x[0] == y[0]:
                bump('tie_within_slot' if x[2] == y[2] else 'tie_across_slots')
        if t == 0 and any(c[3] == eos for c in sel):
            bump('eos_at_t0')
        if t == T - 1 and any(c[3] != eos for c in sel):
            bump('final_by_last_step')
        if done_after >= W and cont:
            bump('stopped_with_continuing_dropped')
        if live * k < W and k < W:
            bump('fewer_candidates_than_beam')
        if np.isneginf(top_lp[base:base + live]).any():
            bump('neg_inf_entry')
        if any(np.isneginf(c[0]) for c in sel):
            bump('neg_inf_selected')
        if live_next == 0:
            tr.setdefault('end_steps', set()).add(t)
    return moved


def history_of(s):
    """The model's buffers as DeviceSpeakerBeam.run returns them (ld_hist at its minimum)."""
    B, W, T, Tp = s['B'], s['beam'], s['T'], s['Tp']
    R = B * W
    t_end = int(s['inst'][:, 2].max())
    return dict(inst=s['inst'].astype(np.int64), done_rec=s['done_rec'], done_score=s['done_score'],
                hist_word=s['hist_word'][:t_end, :R], hist_parent=s['hist_parent'][:t_end, :R],
                hist_score=s['hist_score'][:t_end, :R], hist_attn=s['hist_attn'][:t_end, :R * Tp].reshape(t_end, R, Tp))


def device_model(B, beam, T):
    """The device word loop: sf_speaker_beam_select launch by launch (`model_step`), the decoder replaced by
    lineage_logp; returns what DeviceSpeakerBeam.run returns."""
    R, k = B * beam, min(beam, VOCAB)
    s = new_state(B, beam, T, TP)
    lineage = {b * beam: (b,) for b in range(B)}                     # the word history of every live slot
    for _ in range(T + 2):                                           # (launches past the end change nothing)
        top_w, top_lp = np.full((R, k), EOS, np.int32), np.full((R, k), np.nan, F32)
        alpha = np.full((R, TP), np.nan, F32)
        cur = {}
        for b in range(B):
            for i in range(int(s['inst'][b, 0])):
                r = b * beam + i
                cur[r] = lineage[r] + (int(s['words'][r]),)
                alpha[r] = lineage_alpha(cur[r])
                top_w[r], top_lp[r] = topk(lineage_logp(cur[r]), k)
        lineage = {}
        for b, successors in model_step(s, top_w, top_lp, alpha):
            for p, c in enumerate(successors):
                lineage[b * beam + p] = cur[b * beam + c[2]]
    return history_of(s)


def device_model_whole(B, beam, T):
    """The device word loop as ONE function, as it stood before `model_step` was taken out of it (verbatim): what
    `device_model` has to reproduce."""
    R, k = B * beam, min(beam, VOCAB)
    inst = np.zeros((B, 3), np.int64)
    inst[:, 0] = 1
    lineage = {b * beam: (b,) for b in range(B)}                     # the word history of every live slot
    words = {b * beam: BOS for b in range(B)}
    score = {b * beam: F32(0) for b in range(B)}
    hw, hp = np.full((T, R), -7, np.int32), np.full((T, R), -7, np.int32)
    hs, ha = np.full((T, R), np.nan, F32), np.full((T, R, TP), np.nan, F32)
    done_rec, done_score = np.zeros((B, 2 * beam), np.int32), np.zeros((B, 2 * beam), F32)
    for t in range(T):
        nxt_lineage, nxt_words, nxt_score = {}, {}, {}
        for b in range(B):
            live, n_done, tb = inst[b]
            if live <= 0 or tb >= T:
                continue
            base = b * beam
            cands = []
            for i in range(live):
                lin = lineage[base + i] + (words[base + i],)
                ha[t, base + i] = lineage_alpha(lin)
                tw, tl = topk(lineage_logp(lin), k)
                for j in range(k):
                    cands.append((F32(score[base + i] + tl[j]), i * k + j, i, int(tw[j]), lin))
            cands.sort(key=lambda c: (-c[0], c[1]))
            sel = cands[:beam]
            fin = [c[3] == EOS or t == T - 1 for c in sel]
            cont = [c for c, f in zip(sel, fin) if not f]
            finals = [c for c, f in zip(sel, fin) if f]
            for p, c in enumerate(cont + finals):
                hw[t, base + p], hp[t, base + p], hs[t, base + p] = c[3], base + c[2], c[0]
            for q, c in enumerate(finals):
                done_rec[b, n_done + q] = t * R + base + len(cont) + q
                done_score[b, n_done + q] = c[0]
            n_done += len(finals)
            live = 0 if n_done >= beam else len(cont)
            for p, c in enumerate(cont[:live]):
                nxt_lineage[base + p], nxt_words[base + p], nxt_score[base + p] = c[4], c[3], c[0]
            inst[b] = live, n_done, t + 1
        lineage, words, score = nxt_lineage, nxt_words, nxt_score
        if not lineage:
            break
    t_end = int(inst[:, 2].max())
    return dict(inst=inst, done_rec=done_rec, done_score=done_score, hist_word=hw[:t_end], hist_parent=hp[:t_end],
                hist_score=hs[:t_end], hist_attn=ha[:t_end])


@pytest.mark.parametrize('B,beam,T', [(3, 4, 6), (4, 5, 12), (2, 1, 5), (3, 12, 4)])
def test_device_history_layout_gives_the_host_loop_results(monkeypatch, B, beam, T):
    from speaker_follower_amd import frontier, search
    monkeypatch.setattr(search, 'FlatSpeakerDecoder', FakeFlatDecoder)
    spk = FakeSpeaker(B, T)
    want = frontier.speaker_beam_search(spk, beam, None, None)
    hist = device_model(B, beam, T)
    done, P, W, S, rows = search.speaker_beam_nodes(hist, B, beam)
    att = hist['hist_attn'].reshape(-1, TP)
    got = frontier.speaker_beam_outputs([{'instr_id': 'p%d' % b} for b in range(B)], list(range(B)), done, P, W, S,
                                        rows, beam, lambda r: list(att[r]) if r else [], Tok())
    assert_same(got, want)
    assert sum(len(x) for x in want) == B * beam


@pytest.mark.parametrize('B,beam,T', [(3, 4, 6), (4, 5, 12), (2, 1, 5), (3, 12, 4)])
def test_model_step_reproduces_the_whole_loop_model(B, beam, T):
    """`model_step` driven launch by launch gives what the one-function model gave before it was split: every place the
    contract names, bit for bit (the places it does not name hold the filler of either model and are left out)."""
    got, want = device_model(B, beam, T), device_model_whole(B, beam, T)
    assert np.array_equal(got['inst'], want['inst'])
    assert got['hist_word'].shape == want['hist_word'].shape
    named = want['hist_word'] != -7
    assert np.array_equal(got['hist_word'] != POISON, named)
    for key in ('hist_word', 'hist_parent'):
        assert np.array_equal(got[key][named], want[key][named]), key
    assert np.array_equal(got['hist_score'][named].view(np.int32), want['hist_score'][named].view(np.int32))
    att = ~np.isnan(want['hist_attn'])
    assert np.array_equal(got['hist_attn'].view(np.int32) != POISON, att)
    assert np.array_equal(got['hist_attn'][att].view(np.int32), want['hist_attn'][att].view(np.int32))
    for b in range(B):
        n = int(want['inst'][b, 1])
        assert np.array_equal(got['done_rec'][b, :n], want['done_rec'][b, :n])
        assert np.array_equal(got['done_score'][b, :n].view(np.int32), want['done_score'][b, :n].view(np.int32))
        assert (got['done_rec'][b, n:] == POISON).all()


# ---- the C entry
def _beam_struct(lib_mod, B=4, beam=8, k=8, T=10, Tp=5, eos=2, ld=None, nulls=()):
    R = B * beam
    fields = dict(score=64, words=64, parent=64, inst=64, live_total=64, hist_word=64, hist_parent=64, hist_score=64,
                  hist_attn=64, done_rec=64, done_score=64)
    for n in nulls:
        fields[n] = None
    return lib_mod.SpkBeam(B, beam, k, T, Tp, eos, *(fields[n] for n in (
        'score', 'words', 'parent', 'inst', 'live_total', 'hist_word', 'hist_parent', 'hist_score', 'hist_attn')),
        R * (3 + Tp) if ld is None else ld, fields['done_rec'], fields['done_score'])


def test_beam_select_entry_is_exported_and_bound():
    from speaker_follower_amd import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, 'sf_speaker_beam_select')
    assert 'sf_speaker_beam_select' in _lib.EXPORTS
    assert _lib.lib.sf_speaker_beam_select.argtypes is not None
    assert _lib.ABI_VERSION == 10 and _lib.lib.sf_abi_version() == 10


def test_beam_select_rejects_bad_arguments_without_gpu():
    """Pointers that look valid (never dereferenced: the checks come first), then one bad argument at a time."""
    from speaker_follower_amd import _lib
    sel = _lib.lib.sf_speaker_beam_select
    dev = C.c_void_p(64)
    assert sel(None, dev, dev, dev, None) == 1
    s = _beam_struct(_lib)
    assert sel(C.byref(s), None, dev, dev, None) == 1                      # top_w
    assert sel(C.byref(s), dev, None, dev, None) == 1                      # top_lp
    assert sel(C.byref(s), dev, dev, None, None) == 1                      # hist_attn without alpha
    for n in ('score', 'words', 'parent', 'inst', 'live_total', 'hist_word', 'hist_parent', 'hist_score', 'done_rec',
              'done_score'):
        s = _beam_struct(_lib, nulls=(n,))
        assert sel(C.byref(s), dev, dev, dev, None) == 1, n
    for kw in (dict(k=9, beam=8), dict(k=0), dict(B=0), dict(beam=0, k=0), dict(T=0), dict(Tp=0), dict(eos=-1),
               dict(ld=4 * 8 * 5 - 1), dict(ld=4 * 8 - 1)):
        s = _beam_struct(_lib, **kw)
        assert sel(C.byref(s), dev, dev, dev, None) == 1, kw
    s = _beam_struct(_lib, beam=65, k=65)                                  # wider than one wavefront: unsupported
    assert sel(C.byref(s), dev, dev, dev, None) == 2
    s = _beam_struct(_lib, beam=65, k=66)
    assert sel(C.byref(s), dev, dev, dev, None) == 1


# ---- constructed inputs of the kernel-alone test (tests/test_gpu_choice_kernels.py), checked here for what they reach
VOC = 70                          # >= 64: k = beam_size at every beam the kernel takes
SCENARIOS = ('to_the_last_step', 'eos_early', 'short_lists')


def scenario_shape(name, B, beam, Tp=4):
    """(k, T, with_attn, ld_hist) of a scenario: the attention history present and absent, ld_hist at and above its
    minimum, k = beam_size and k < beam_size."""
    R = B * beam
    if name == 'to_the_last_step':
        return min(beam, VOC), 5, True, R * Tp + 8
    if name == 'eos_early':
        return min(beam, VOC), 7, False, R
    return max(1, min(beam - 1, 2)), 7, True, R * Tp


def scenario_inputs(rng, s, k, name, step):
    """top_w / top_lp / alpha of one launch on state `s`.  Live slots get what sf_logprob_topk gives for a row of coarse
    log-probabilities (multiples of 0.5: the float32 sums tie exactly), some rows perturbed; dead slots get junk that
    would win the selection if it were read."""
    B, W, Tp, eos = s['B'], s['beam'], s['Tp'], s['eos']
    R = B * W
    top_w = rng.integers(0, VOC, (R, k)).astype(np.int32)
    top_lp = (rng.standard_normal((R, k)) * 3 + 50).astype(F32)
    alpha = rng.random((R, Tp)).astype(F32)
    for b in range(B):
        for i in range(int(s['inst'][b, 0]) if s['inst'][b, 2] < s['T'] else 0):
            lp = (-0.5 * rng.integers(0, 4, VOC)).astype(F32)
            if rng.random() < 0.3:
                lp = (lp + rng.standard_normal(VOC).astype(F32) * F32(0.37)).astype(F32)
            if name == 'to_the_last_step':
                lp[eos] = F32(-60.0)                          # never among the best: the last step makes the finals
            elif step <= 1:                                   # EOS the best word of every live slot of the even instances
                lp[eos] = F32(0.5) if b % 2 == 0 else F32(-9.0)
            else:
                lp[eos] = F32(0.5 * rng.integers(0, 3)) if step >= 2 + b % 3 else F32(-9.0)
            if name == 'short_lists' and (step + b + i) % 2 == 0:     # fewer finite words than k: -inf inside the list
                gone = rng.permutation(VOC)[1 + (step + b) % k:]
                lp[gone] = -np.inf
            top_w[b * W + i], top_lp[b * W + i] = topk(lp, k)
    return top_w, top_lp, alpha


def scenario_expectations(trace, B, beam):
    """What the scenarios of one (B, beam) must have reached, on the model's own trace."""
    need = ['eos_at_t0', 'final_by_last_step', 'noop', 'neg_inf_entry'] if beam > 1 else ['eos_at_t0', 'final_by_last_step', 'noop']
    if beam >= 3:
        need += ['tie_across_slots', 'tie_within_slot', 'stopped_with_continuing_dropped', 'fewer_candidates_than_beam']
    missing = [n for n in need if not trace.get(n)]
    assert not missing, (B, beam, missing, trace)
    if B > 1:
        assert len(trace['end_steps']) > 1, 'every instance ended at the same step'


@pytest.mark.parametrize('B,beam', [(1, 1), (1, 3), (64, 3), (1, 40), (5, 40), (1, 64), (3, 64)])
def test_scenarios_reach_every_case_of_the_contract(B, beam):
    """The model alone over the constructed inputs (the GPU test runs the same at B = 64 as well): every case the
    kernel-alone test is there for is reached, and launches after the end leave every buffer as it was."""
    trace = {}
    for name in SCENARIOS:
        rng = np.random.default_rng([B, beam, SCENARIOS.index(name)])
        k, T, with_attn, ld = scenario_shape(name, B, beam)
        s = new_state(B, beam, T, 4, with_attn=with_attn, ld=ld)
        for step in range(T + 2):
            before = {n: v.copy() for n, v in s.items() if isinstance(v, np.ndarray)}
            ended = (s['inst'][:, 0] == 0).all()
            top_w, top_lp, alpha = scenario_inputs(rng, s, k, name, step)
            model_step(s, top_w, top_lp, alpha if with_attn else None, trace)
            if ended:
                assert all(np.array_equal(before[n].view(np.int32), s[n].view(np.int32)) for n in before)
        assert (s['inst'][:, 0] == 0).all() and (s['inst'][:, 2] <= T).all()
        assert ((s['inst'][:, 1] >= 1) & (s['inst'][:, 1] < 2 * beam)).all()
    scenario_expectations(trace, B, beam)
