"""CPU: the host side of the speaker's device beam search (search.DeviceSpeakerBeam / sf_speaker_beam_select).

* frontier.speaker_beam_outputs -- the result assembly the host and device word loops share -- gives what the host
  loop's own tail gave before it was factored out, on synthetic hypotheses with exact score ties;
* the device loop's history layout (include/sf_hip.h: sf_speaker_beam_select), produced by a step-by-step model of the
  kernel and read back through search.speaker_beam_nodes, gives the host loop's results (frontier.speaker_beam_search
  over a stand-in decoder whose log-probabilities are a function of the word history, with many ties);
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


def device_model(B, beam, T):
    """sf_speaker_beam_select step by step (include/sf_hip.h layout), the decoder replaced by lineage_logp; returns
    what DeviceSpeakerBeam.run returns."""
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
    assert _lib.ABI_VERSION == 9 and _lib.lib.sf_abi_version() == 9


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
