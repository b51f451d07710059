"""GPU: sf_bleu_counts (csrc/sf_bleu.hip) alone, `SpeakerEvaluation.score_results` counting on the device, and
`SpeakerEvaluation.score_speaker` end to end.  Every comparison is exact: integers against
speaker_evaluation.bleu_count_rows (the kernel's specification), `==` on the doubles of a summary.

* the kernel against bleu_count_rows: hypothesis lengths 0..5, 63, 64, 65, 80 and the limit, reference lengths 0, 1, 3,
  4, 64, 65 and the limit, 1..4 references, ids 0 and 65 535, 1 / 63 / 64 / 65 / 257 paths, slots with -1 interleaved,
  both hypothesis forms (packed; a decode's [S, B] matrix as int64 and int16 with EOS at 0, in the middle, at S - 1 and
  absent, a PAD inside, a remap that is not the identity), 2 000 random paths over four words
* the limits, lowered through sf_debug_bleu_limits: just inside exact, one over SF_ERR_UNSUPPORTED with nothing
  written, score_results still the golden numbers through the host merge; a bad slot and an id outside the dictionary
  raise err[0] and write nothing
* score_results on the device == the reference's recorded summaries (tests/golden/g16_speaker_bleu.json.gz)
* score_speaker == agent.test() + score_results(agent.results): a speaker over the fixture connectivity, a synthetic
  feature table and seeded weights.  Only 2 of the split's 260 paths lie in the 8 committed scans; 28 more routes are
  drawn on those scans and carry the path ids, instruction texts and token ids of other paths of the split (one of
  them with four instructions), so that the references are real: 30 paths, 91 items, 6 minibatches of 16, the last
  one wrapping."""
import ctypes as C
import contextlib
import io
import os
import random
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import speaker_bleu_cases as cases                                  # noqa: E402
import r2r_val_seen as VS                                           # noqa: E402

from speaker_follower_amd import speaker_evaluation as se           # noqa: E402

DEV = torch.device('cuda', 0)
FX = cases.load()
SENTINEL = -7
BIG = 65535


def launch(refs, hyps=None, slots=None, n_slots=None, n_dict=BIG + 1, words=None, eos=2, remap=None, max_hyp=None,
           max_ref=None):
    """sf_bleu_counts once.  refs: per slot R id lists; hyps: id lists (packed form) or `words` [S, B] (matrix form,
    int64 or int16) with `remap`.  Returns (status, rows [n_slots, 10] over sentinels, sums, err)."""
    from speaker_follower_amd import _lib
    R = len(refs[0])
    n_slots = len(refs) if n_slots is None else n_slots
    B = len(hyps) if words is None else words.shape[1]
    slots = np.arange(B, dtype=np.int32) if slots is None else np.asarray(slots, np.int32)
    r_ids, r_off = se._packed([r for rs in refs for r in rs])
    h_ids, h_off = se._packed(hyps if words is None else [[]] * B)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)                      # noqa: E731
    d = dict(r_ids=up(r_ids), r_off=up(r_off), h_ids=up(h_ids), h_off=up(h_off), slot=up(slots))
    rows = torch.full((n_slots, 10), SENTINEL, dtype=torch.int32, device=DEV)
    sums = torch.zeros(10, dtype=torch.int64, device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    b = _lib.BleuBatch(n_hyps=B, n_slots=n_slots, n_refs=R, n_dict=n_dict,
                       max_hyp=int(np.diff(h_off).max()) if max_hyp is None else max_hyp,
                       max_ref=int(np.diff(r_off).max()) if max_ref is None else max_ref,
                       ref_ids=d['r_ids'].data_ptr(), ref_off=d['r_off'].data_ptr(), slot=d['slot'].data_ptr(),
                       rows=rows.data_ptr(), sums=sums.data_ptr())
    if words is None:
        b.hyp_ids, b.hyp_off = d['h_ids'].data_ptr(), d['h_off'].data_ptr()
    else:
        d['words'], d['remap'] = up(words), up(np.asarray(remap, np.int32))
        b.words, b.remap, b.S, b.eos, b.n_vocab = d['words'].data_ptr(), d['remap'].data_ptr(), words.shape[0], eos, len(remap)
        b.word_bytes = words.dtype.itemsize
    status = _lib.lib.sf_bleu_counts(C.byref(b), C.c_void_p(err.data_ptr()),
                                     C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return status, rows.cpu().numpy(), sums.cpu().numpy(), int(err.item())


def check(refs, hyps, slots=None, n_slots=None, **kw):
    """The launch against bleu_count_rows: written rows equal, rows nobody owns untouched, sums = the written rows."""
    status, rows, sums, err = launch(refs, hyps, slots=slots, n_slots=n_slots, **kw)
    assert status == 0 and err == 0
    slots = list(range(len(hyps))) if slots is None else list(slots)
    live = [(b, s) for b, s in enumerate(slots) if s >= 0]
    want = se.bleu_count_rows([refs[s] for _, s in live], [hyps[b] for b, _ in live])
    for (b, s), w in zip(live, want):
        assert rows[s].tolist() == w.tolist(), (b, s, rows[s].tolist(), w.tolist())
    idle = sorted(set(range(len(rows))) - {s for _, s in live})
    assert (rows[idle] == SENTINEL).all()
    assert sums.tolist() == want.sum(0, dtype=np.int64).tolist()
    return want


def sentence(rng, n, alphabet):
    return [int(alphabet[i]) for i in rng.integers(len(alphabet), size=n)]


def test_counts_at_every_length_edge_equal_the_host_rows():
    rng = np.random.default_rng(1)
    alphabet = [0, 5, 9, BIG]                                       # (dense in repeats; the smallest and largest id)
    hyp_lens = [0, 1, 2, 3, 4, 5, 63, 64, 65, 80, 256]
    ref_lens = [0, 1, 3, 4, 64, 65, 512]
    for R in (1, 2, 3, 4):
        refs, hyps = [], []
        for h in hyp_lens:
            for r in ref_lens:
                lens = [r] + [int(ref_lens[i]) for i in rng.integers(len(ref_lens), size=R - 1)]
                refs.append([sentence(rng, n, alphabet) for n in lens])
                hyps.append(sentence(rng, h, alphabet))
        # a hypothesis that IS one of its references, and one whose words no reference holds
        refs.append([sentence(rng, 80, alphabet) for _ in range(R)])
        hyps.append(list(refs[-1][R - 1]))
        refs.append([sentence(rng, 30, alphabet[:2]) for _ in range(R)])
        hyps.append(sentence(rng, 30, alphabet[2:]))
        want = check(refs, hyps)
        assert want[-2][:4].tolist() == want[-2][4:8].tolist() and want[-1][:4].tolist() == [0, 0, 0, 0]
        assert (want[:, 0] > 0).any() and (want[:, 3] > 0).any()


@pytest.mark.parametrize('n_paths', [1, 63, 64, 65, 257])
def test_path_counts_and_interleaved_empty_slots(n_paths):
    rng = np.random.default_rng(100 + n_paths)
    alphabet = list(range(12))
    refs = [[sentence(rng, int(rng.integers(0, 40)), alphabet) for _ in range(3)] for _ in range(n_paths)]
    B = n_paths + n_paths // 2 + 1                                  # more hypotheses than paths: the others hold -1
    slots = np.full(B, -1, np.int64)
    slots[rng.permutation(B)[:n_paths]] = rng.permutation(n_paths)
    hyps = [sentence(rng, int(rng.integers(0, 45)), alphabet) for _ in range(B)]
    check(refs, hyps, slots=slots.tolist(), n_slots=n_paths)
    # every slot owned, in order; and two slots behind the paths that nobody owns
    check(refs, hyps[:n_paths])
    check(refs + [[[1], [2], [3]]] * 2, hyps[:n_paths], slots=list(range(n_paths)), n_slots=n_paths + 2)


def test_two_thousand_random_paths_over_four_words():
    rng = np.random.default_rng(7)
    alphabet = [3, 4, 5, 6]
    refs = [[sentence(rng, int(rng.integers(0, 36)), alphabet) for _ in range(3)] for _ in range(2000)]
    hyps = [sentence(rng, int(rng.integers(0, 36)), alphabet) for _ in range(2000)]
    want = check(refs, hyps, n_dict=7)
    assert (want[:, :4] < want[:, 4:8]).any() and (want[:, 3] > 0).any()


@pytest.mark.parametrize('dtype', [np.int64, np.int16])
def test_word_matrix_form_equals_decode_sentence(dtype):
    rng = np.random.default_rng(11)
    S, B, V, EOS, PAD = 20, 70, 50, 2, 0
    # not the identity: dictionary ids 100 .. 247; word 7 is two BLEU words, word 9 none, the others one
    remap = np.stack(((rng.permutation(V) * 3 + 100), np.full(V, -1)), axis=1).astype(np.int32)
    remap[7, 1], remap[9] = 250, (-1, -1)
    words = rng.integers(3, V, size=(S, B))
    words[rng.integers(S, size=B), np.arange(B)] = PAD              # a PAD does not end a sentence
    ends = {0: 0, 1: S // 2, 2: S - 1, 3: None, 4: 1, 5: 3}         # EOS at 0, in the middle, at S - 1, absent
    for b in range(B):
        e = ends.get(b, int(rng.integers(0, S + 1)))
        if e is not None and e < S:
            words[e:, b] = rng.integers(0, V, size=S - e)           # (whatever a decode leaves behind the EOS)
            words[e, b] = EOS
    words[:, 3] = np.arange(10, 10 + S)                             # no EOS and the two-word entry: S + 1 BLEU words
    words[5, 3], words[1, 2] = 7, 9
    hyps = []
    for b in range(B):
        col = words[:, b].tolist()
        hyps.append([int(i) for w in (col[:col.index(EOS)] if EOS in col else col) for i in remap[w] if i >= 0])
    assert len(hyps[0]) == 0 and any(len(h) > S for h in hyps) and (words[:S // 2] == 9).any()
    pool = sorted(set(remap[:, 0].tolist()) - {-1})
    slots = rng.permutation(B).tolist()
    refs = [None] * B
    for b, h in enumerate(hyps):                                    # (references that share words with their hypothesis)
        refs[slots[b]] = [sentence(rng, int(rng.integers(1, 30)), pool[:8] + h[:6]) for _ in range(2)]
    slots[7] = slots[40] = -1
    status, rows, sums, err = launch(refs, words=words.astype(dtype), eos=EOS, remap=remap, slots=slots, n_dict=300)
    assert status == 0 and err == 0
    live = [(b, s) for b, s in enumerate(slots) if s >= 0]
    want = se.bleu_count_rows([refs[s] for _, s in live], [hyps[b] for b, _ in live])
    for (b, s), w in zip(live, want):
        assert rows[s].tolist() == w.tolist(), (b, s)
    assert sums.tolist() == want.sum(0, dtype=np.int64).tolist() and (want[:, 0] > 0).any()
    # a word outside the vocabulary, a remap entry outside the dictionary: err, and that row is not written
    bad = words.copy()
    bad[0, 5] = V
    status, rows, _, err = launch(refs, words=bad.astype(dtype), eos=EOS, remap=remap, n_dict=300)
    assert status == 0 and err == 1 and (rows[5] == SENTINEL).all() and (rows[6] != SENTINEL).all()
    status, rows, _, err = launch(refs, words=words.astype(dtype), eos=EOS, remap=remap, n_dict=int(remap.max()))
    assert status == 0 and err == 1 and (rows == SENTINEL).any()


def test_limits_refusals_and_fault_word():
    from speaker_follower_amd import _lib
    lib = _lib.lib
    assert se.bleu_limits() == (65536, 256, 512, 4)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.sf_bleu_counts(None, None, st) == _lib.SF_ERR_ARG
    rng = np.random.default_rng(3)
    alphabet = [0, 1, 2, 99]
    refs = [[sentence(rng, 12, alphabet), sentence(rng, 5, alphabet)] for _ in range(3)]
    hyps = [sentence(rng, 10, alphabet), sentence(rng, 9, alphabet), []]
    # above the compile-time limits: refused, nothing written
    over = [sentence(rng, 257, alphabet)] + hyps[1:]
    status, rows, sums, err = launch(refs, over)
    assert status == _lib.SF_ERR_UNSUPPORTED and (rows == SENTINEL).all() and not sums.any() and err == 0
    status, rows, _, _ = launch([[sentence(rng, 513, alphabet)]] * 3, hyps)
    assert status == _lib.SF_ERR_UNSUPPORTED and (rows == SENTINEL).all()
    status, rows, _, _ = launch([[[1]] * 5] * 3, hyps)
    assert status == _lib.SF_ERR_UNSUPPORTED and (rows == SENTINEL).all()
    assert launch(refs, hyps, n_dict=65537)[0] == _lib.SF_ERR_UNSUPPORTED
    lib.sf_debug_bleu_limits(100, 10, 12, 2)
    try:
        assert se.bleu_limits() == (100, 10, 12, 2)
        check(refs, hyps, n_dict=100)                               # just inside every limit: exact
        for kw, r, h in ((dict(n_dict=101), refs, hyps),
                         (dict(n_dict=100), refs, [sentence(rng, 11, alphabet)] + hyps[1:]),
                         (dict(n_dict=100), [[sentence(rng, 13, alphabet), [1]]] * 3, hyps),
                         (dict(n_dict=100), [[[1], [2], [0]]] * 3, hyps)):
            status, rows, sums, err = launch(r, h, **kw)
            assert status == _lib.SF_ERR_UNSUPPORTED and (rows == SENTINEL).all() and not sums.any(), kw
        # host copies that understate the lengths: the kernel sees the real ones, writes nothing for them, raises err
        status, rows, _, err = launch(refs, [sentence(rng, 11, alphabet)] + hyps[1:], n_dict=100, max_hyp=10)
        assert status == 0 and err == 1 and (rows[0] == SENTINEL).all() and (rows[1] != SENTINEL).all()
        # score_results with most paths above the lowered limits: the golden numbers through the host merge
        lib.sf_debug_bleu_limits(0, 25, 40, 0)
        case = FX['sets'][0]
        ev, summary = golden_on_device(case, '3')
        n_host = len(ev.counts['on_host'])
        assert 0 < n_host < 260
        lib.sf_debug_bleu_limits(300, 0, 0, 0)                      # the dictionary fills up part of the way through
        ev, summary = golden_on_device(case, '3')
        assert 0 < len(ev.counts['on_host']) < 260
        lib.sf_debug_bleu_limits(0, 0, 0, 2)                        # three references per path: everything on the host
        ev, summary = golden_on_device(case, '3')
        assert len(ev.counts['on_host']) == 260
    finally:
        lib.sf_debug_bleu_limits(0, 0, 0, 0)
    assert se.bleu_limits() == (65536, 256, 512, 4)
    # a slot outside its array, an id outside the dictionary: err[0], nothing written for that hypothesis
    for slots in ([0, 3, 2], [0, -2, 2]):
        status, rows, sums, err = launch(refs, hyps, slots=slots)
        assert status == 0 and err == 1 and (rows[1] == SENTINEL).all() and (rows[0] != SENTINEL).all()
    status, rows, sums, err = launch([[[99, 1, 2], [0]]] * 3, hyps, n_dict=99)
    assert status == 0 and err == 1 and (rows == SENTINEL).all() and not sums.any()
    status, rows, sums, err = launch(refs, [[0, -1, 2]] + hyps[1:])
    assert status == 0 and err == 1 and (rows[0] == SENTINEL).all() and (rows[1] != SENTINEL).all()
    with pytest.raises(RuntimeError, match='sf_bleu_counts'):
        se._device_rows([[0, 1]], [[5]], 1, 3, DEV)


# ------------------------------------------------------------------------------------------ score_results
def golden_on_device(case, ipp):
    want = case['want'][ipp]
    ev = se.SpeakerEvaluation(items=FX['items'], splits=['sub_val_seen'], instructions_per_path=int(ipp), device=DEV)
    printed = io.StringIO()
    with contextlib.redirect_stdout(printed), np.errstate(all='ignore'):
        summary, replaced = ev.score_results(cases.build_results(FX['items'], case))
    for k, v in want['summary'].items():
        got = float(summary[k])
        assert (np.isnan(got) if v is None else got == v), (case['name'], ipp, k, got, v)
    assert cases.digest([r['instructions'][0] for r in replaced]) == want['replaced'] and printed.getvalue() == want['printed']
    return ev, summary


@pytest.mark.parametrize('name', [c['name'] for c in FX['sets']])
def test_score_results_on_the_device_equals_the_reference(name):
    case = next(c for c in FX['sets'] if c['name'] == name)
    for ipp in sorted(case['want']):
        ev, _ = golden_on_device(case, ipp)
        assert ev.counts['on_host'] == []
        host = se.SpeakerEvaluation(items=FX['items'], instructions_per_path=int(ipp), device='cpu')
        with contextlib.redirect_stdout(io.StringIO()), np.errstate(all='ignore'):
            host.score_results(cases.build_results(FX['items'], case))
        assert sorted(host.counts['rows']) == sorted(ev.counts['rows']) and len(ev.counts['rows']) in (260, 2)
        for pid, row in host.counts['rows'].items():
            assert ev.counts['rows'][pid].tolist() == row.tolist(), pid
        assert ev.counts['sums'].tolist() == host.counts['sums'].tolist()


# ------------------------------------------------------------------------------------------ score_speaker
CONN = os.path.join(cases.ROOT, 'tests', 'golden', 'connectivity')
BATCH, INSTRUCTION_LEN, EPISODE_LEN = 16, 24, 6


class VocabTokenizer:
    """utils.Tokenizer.decode_sentence (utils.py:109-118) over the fixture's vocabulary."""

    def __init__(self, vocab):
        self.vocab = list(vocab)

    def decode_sentence(self, encoding, break_on_eos=False, join=True):
        sentence = []
        for ix in encoding:
            if ix == (2 if break_on_eos else 0):
                break
            sentence.append(self.vocab[ix])
        return ' '.join(sentence) if join else sentence


EOS_LIFT = 0.32                          # (measured: 13 empty sentences, 3 of 16 words, 75 that never end)


def build_speaker_world(eos_lift=EOS_LIFT):
    from speaker_follower_amd.build import build_sim
    build_sim(verbose=False)
    from speaker_follower_amd import agents, env as envm, features, model, synth
    have = sorted(f.split('_')[0] for f in os.listdir(CONN) if f.endswith('_connectivity.json'))
    _, vs = VS.load_items()
    geometry = {p['path_id']: p for p in vs['paths']}
    inside = [it for it in FX['items'] if it['scan'] in have]
    scans = sorted({it['scan'] for it in inside}) + [s for s in have if s not in {it['scan'] for it in inside}][:1]
    graphs = {s: envm.NavGraph(os.path.join(CONN, s + '_connectivity.json')) for s in scans}
    outside = [it for it in FX['items'] if it['scan'] not in have]
    four = [it for it in outside if len(it['instructions']) == 4][:1]
    borrowed = four + [it for it in outside if len(it['instructions']) == 3][:28 - len(four)]
    routes = envm.random_items(graphs, len(borrowed), np.random.default_rng(16))
    paths, items = [], []
    for it in inside:
        g = geometry[it['path_id']]
        paths.append(dict(it, path=g['path'], heading=g['heading']))
    for it, route in zip(borrowed, routes):
        paths.append(dict(it, scan=route['scan'], path=route['path'], heading=route['heading']))
    for p in paths:
        for j, enc in enumerate(geometry[p['path_id']]['instr_encodings']):
            items.append(dict(scan=p['scan'], path_id=p['path_id'], path=p['path'], heading=p['heading'],
                              instr_id='%s_%d' % (p['path_id'], j), instructions=p['instructions'][j],
                              instr_encoding=np.asarray(enc, np.int64)))
    row_of, n = {}, 0
    for s in scans:
        for v in graphs[s].ids:
            row_of[s + '_' + v] = n
            n += 1
    table = synth.feature_table(16, n)
    state = random.getstate()
    env = envm.R2RIndexEnv(items, row_of, CONN, batch_size=BATCH, scans=scans)
    env.tokenizer = VocabTokenizer(FX['vocab'])
    d = synth.FULL
    assert len(FX['vocab']) == d.vocab
    w_enc, w_dec = synth.speaker_weights(216)
    # seeded weights say nothing: lift <EOS> and the ten most frequent words ('the', '.', 'and', 'walk', ...) so that
    # the sentences end at different lengths and share words with their references
    w_dec['decoder2action.bias'][3:13] += np.float32(0.25)
    w_dec['decoder2action.bias'][2] += np.float32(eos_lift)
    senc = model.SpeakerEncoderLSTM(d.feat, d.feat, d.hidden, 0.5)
    sdec = model.SpeakerDecoderLSTM(d.vocab, d.word, d.hidden, 0.5, glove=w_dec['embedding.weight'])
    senc.load_state_dict({k: torch.tensor(v) for k, v in w_enc.items()})
    sdec.load_state_dict({k: torch.tensor(v) for k, v in w_dec.items()})
    spk = agents.Seq2SeqSpeaker(env, '/tmp/sf_speaker_evaluation.json', senc.cuda().eval(), sdec.cuda().eval(),
                                INSTRUCTION_LEN, max_episode_len=EPISODE_LEN)
    random.setstate(state)
    spk.store = features.FeatureStore(table)
    spk.sweep_test_after = 0             # test() decodes through the sweep's graphs too: the same float scores
    print('speaker world: %d of the split\'s paths in the committed scans, %d paths in all, %d items, batches of %d'
          % (len(inside), len(paths), len(items), BATCH))
    assert len(paths) == 30 and len(items) == 91 and len(items) % BATCH != 0
    return dict(env=env, spk=spk, paths=paths, items=items, ev=se.SpeakerEvaluation(env=env, device=DEV))


@pytest.fixture(scope='module')
def speaker_world():
    return build_speaker_world()


class Rewind:
    """The environment's item order and `random` as they were: two walks from the same state."""

    def __init__(self, env):
        self.env, self.data, self.state = env, list(env.data), random.getstate()

    def __call__(self):
        self.env.data[:] = self.data
        random.setstate(self.state)

    def after(self):
        return self.env.ix, [it['instr_id'] for it in self.env.data], random.random()


def test_score_speaker_equals_test_plus_score_results(speaker_world):
    w = speaker_world
    spk, ev, env = w['spk'], w['ev'], w['env']
    assert len(ev.gt) == 30 and len(ev.instr_ids) == 90             # ('<path>_3' of the four-instruction path is not scored)
    rewind = Rewind(env)
    results = spk.test(use_dropout=False, feedback='argmax')
    summary, replaced = ev.score_results(results)
    rows = {pid: r.tolist() for pid, r in ev.counts['rows'].items()}
    losses, words = list(spk.losses), {k: list(v['words']) for k, v in results.items()}
    assert len(results) == 91 and ev.counts['on_host'] == [] and len(losses) == 6
    end = rewind.after()
    rewind()
    sweeps, fallbacks = ev.sweeps, ev.fallbacks
    got, nothing = ev.score_speaker(spk)
    assert rewind.after() == end                                    # env.ix, the item order, the next random.random()
    assert nothing is None and spk.results == {}
    assert ev.last_host_syncs == 1 and ev.fallbacks == fallbacks == 0 and ev.sweeps == sweeps + 1
    print('score_speaker: %s over %d paths in %d minibatches; hypothesis lengths %s'
          % (got, len(rows), len(losses), sorted({r[8] for r in rows.values()})))
    assert set(got) == {'model_score', 'bleu', 'unpenalized_bleu'}
    assert len({r[8] for r in rows.values()}) > 1 and sum(r[0] for r in rows.values()) > 0   # EOS met; words shared
    for k in got:
        assert got[k] == summary[k], (k, got[k], summary[k])       # == on doubles
    assert spk.losses == losses
    # every path once, although the last minibatch wraps into items already decoded
    assert sorted(ev.counts['rows']) == sorted(rows) and len(rows) == 30
    for pid, r in rows.items():
        assert ev.counts['rows'][pid].tolist() == r, pid
    first = {}
    for k, v in words.items():
        if k in ev.instr_ids:
            first.setdefault(int(k.split('_')[0]), v)
    host = se.bleu_count_rows([ev._references(p) for p in sorted(first)], [se.bleu_words(first[p]) for p in sorted(first)])
    assert [ev.counts['rows'][p].tolist() for p in sorted(first)] == host.tolist()
    assert ev.counts['sums'].tolist() == host.sum(0, dtype=np.int64).tolist()
    # keep_results: test()'s results, in its order, and the generated instructions
    rewind()
    kept, kept_replaced = ev.score_speaker(spk, keep_results=True)
    assert ev.last_host_syncs == 1 and kept == got
    assert list(spk.results) == list(results)
    assert {k: list(v['words']) for k, v in spk.results.items()} == words
    assert all(spk.results[k]['score'] == results[k]['score'] for k in results)
    assert kept_replaced == replaced
    # the loop over rollout() (test() below its sweep threshold) generates the same words: the same BLEU
    rewind()
    spk.sweep_test_after = 10 ** 9
    try:
        by_loop, _ = ev.score_results(spk.test(use_dropout=False, feedback='argmax'))
    finally:
        spk.sweep_test_after = 0
    print('test() as a loop over rollout(): %s' % by_loop)
    assert (by_loop['bleu'], by_loop['unpenalized_bleu']) == (got['bleu'], got['unpenalized_bleu'])
    rewind()


def test_score_speaker_falls_back_with_dropout(speaker_world):
    w = speaker_world
    spk, ev = w['spk'], w['ev']
    rewind = Rewind(w['env'])
    before, sweeps = ev.fallbacks, ev.sweeps
    try:
        got, replaced = ev.score_speaker(spk, use_dropout=True)
        assert ev.fallbacks == before + 1 and ev.sweeps == sweeps
        again, again_replaced = ev.score_results(spk.results)      # what the fall-back scored is what test() left
        assert len(spk.results) == 91
        for k in got:
            assert got[k] == again[k]
        assert replaced == again_replaced
    finally:
        for m in (spk.encoder, spk.decoder):
            m.eval()
        rewind()
