"""A speaker's validation on val-seen (782 instructions / 260 paths, batch 100, seeded weights, the instruction texts
of tests/golden/g16_speaker_bleu.json.gz as references) in one process, after a warm-up, taking turns:
Seq2SeqSpeaker.test() alone -- as the loop over rollout() and as the sweep it becomes after `sweep_test_after`
minibatches --, SpeakerEvaluation.score_speaker (the sweep with sf_bleu_counts behind every minibatch, one host sync),
and score_results on kept results, counting on the host and on the device.  Median of 7 with min / max.

    python tools/speaker_eval_time.py [--out profiles/speaker_evaluation_sweep.txt]"""
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np                                                           # noqa: E402
import torch                                                                 # noqa: E402
import r2r_val_seen as VS                                                    # noqa: E402
import speaker_bleu_cases as cases                                           # noqa: E402
from speaker_follower_amd import agents, features, model, synth             # noqa: E402
from speaker_follower_amd import speaker_evaluation as se                   # noqa: E402

REPS, BATCH, INSTRUCTION_LEN, EPISODE_LEN = 7, 100, 80, 10
out_path = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


class VocabTokenizer:
    def __init__(self, vocab):
        self.vocab = list(vocab)

    def decode_sentence(self, encoding, break_on_eos=False, join=True):
        sentence = []
        for ix in encoding:
            if ix == (2 if break_on_eos else 0):
                break
            sentence.append(self.vocab[ix])
        return ' '.join(sentence) if join else sentence


fx = cases.load()
text = {it['path_id']: it['instructions'] for it in fx['items']}
items, _ = VS.load_items()
for it in items:
    it['instructions'] = text[it['path_id']][int(it['instr_id'].split('_')[1])]
state = random.getstate()
env, row_of, n_rows = VS.build_env(items, batch_size=BATCH)
env.tokenizer = VocabTokenizer(fx['vocab'])
d = synth.FULL
w_enc, w_dec = synth.speaker_weights(216)
w_dec['decoder2action.bias'][2:13] += np.float32(0.25)                       # (sentences that end, made of frequent words)
senc = model.SpeakerEncoderLSTM(d.feat, d.feat, d.hidden, 0.5)
sdec = model.SpeakerDecoderLSTM(d.vocab, d.word, d.hidden, 0.5, glove=w_dec['embedding.weight'])
senc.load_state_dict({k: torch.tensor(v) for k, v in w_enc.items()})
sdec.load_state_dict({k: torch.tensor(v) for k, v in w_dec.items()})
spk = agents.Seq2SeqSpeaker(env, '/tmp/sf_speaker_eval_time.json', senc.cuda().eval(), sdec.cuda().eval(),
                            INSTRUCTION_LEN, max_episode_len=EPISODE_LEN)
random.setstate(state)
spk.store = features.FeatureStore(synth.feature_table(21, n_rows))
ev = se.SpeakerEvaluation(env=env)
ev_host = se.SpeakerEvaluation(env=env, device='cpu')
data0, state0 = list(env.data), random.getstate()


def rewind():
    env.data[:] = data0
    random.setstate(state0)


def test_loop():
    spk.sweep_test_after = 10 ** 9
    return spk.test(use_dropout=False, feedback='argmax')


def test_sweep():
    spk.sweep_test_after = 0
    return spk.test(use_dropout=False, feedback='argmax')


def sweep():
    return ev.score_speaker(spk)[0]


rewind()
kept = dict(test_sweep())


def score_host():
    return ev_host.score_results(kept)[0]


def score_device():
    return ev.score_results(kept)[0]


import contextlib                                                            # noqa: E402
import io                                                                    # noqa: E402
fns = (test_loop, test_sweep, sweep, score_host, score_device)
with contextlib.redirect_stdout(io.StringIO()):                              # (score_results reports mismatching duplicates)
    for fn in fns + fns:                                                     # warm-up: captures, tables, the dictionary
        rewind()
        fn()
    times = {fn: [] for fn in fns}
    last = {}
    for rep in range(REPS):
        for fn in fns:
            rewind()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last[fn] = fn()
            torch.cuda.synchronize()
            times[fn].append(time.perf_counter() - t0)
rewind()
assert ev.fallbacks == 0 and ev.last_host_syncs == 1
assert last[sweep] == last[score_host] == last[score_device], (last[sweep], last[score_host], last[score_device])
for name, fn in (('Seq2SeqSpeaker.test() alone, the loop over rollout()', test_loop),
                 ('Seq2SeqSpeaker.test() alone, as a sweep', test_sweep),
                 ('SpeakerEvaluation.score_speaker (one sweep, one host sync)', sweep),
                 ('score_results on kept results, counted on the host', score_host),
                 ('score_results on kept results, counted on the device', score_device)):
    ms = [x * 1e3 for x in times[fn]]
    say('%-62s median %.2f ms  min %.2f  max %.2f  (%d runs, %d instructions, %d minibatches of %d, %d words)'
        % (name, statistics.median(ms), min(ms), max(ms), REPS, len(items), len(spk.losses), BATCH, INSTRUCTION_LEN))
say('summary every way: %s; sums %s' % (last[sweep], ev.counts['sums'].tolist()))
if out_path:
    with open(out_path, 'w') as f:
        f.write('\n'.join(lines) + '\n')
