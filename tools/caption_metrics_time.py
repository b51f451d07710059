"""What the caption metrics (ROUGE-L and CIDEr-D, `SpeakerEvaluation(..., caption_metrics=True)`) cost, on the world of
tools/speaker_eval_time.py: a speaker's validation on val-seen (782 instructions / 260 paths, batch 100, seeded
weights, the instruction texts of tests/golden/g16_speaker_bleu.json.gz as references), in one process, after a
warm-up, taking turns: score_speaker with the switch off and on (sf_caption_scores behind every minibatch, next to
sf_bleu_counts; still one host sync), and score_results on kept results with the parts formed on the host and on the
device.  Median of 7 with min / max; the largest difference between the device's and the host's per-path numbers.

    python tools/caption_metrics_time.py [--out profiles/caption_metrics_sweep.txt]
    python tools/caption_metrics_time.py --off-only [--root <another checkout>] [--label parent] [--out ... --append]

--off-only times score_speaker with the switch off alone; with --root it imports the package of another checkout (one
that need not know the switch): the parent commit's own tree, to show that the off path did not move."""
import contextlib
import inspect
import io
import os
import random
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def option(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


ROOT = os.path.abspath(option('--root', HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np                                                           # noqa: E402
import torch                                                                 # noqa: E402
import r2r_val_seen as VS                                                    # noqa: E402
import speaker_bleu_cases as cases                                           # noqa: E402
from speaker_follower_amd import agents, features, model, synth             # noqa: E402
from speaker_follower_amd import speaker_evaluation as se                   # noqa: E402

REPS, BATCH, INSTRUCTION_LEN, EPISODE_LEN = 7, 100, 80, 10
out_path, label, off_only = option('--out'), option('--label', 'repo'), '--off-only' in sys.argv
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
spk = agents.Seq2SeqSpeaker(env, '/tmp/sf_caption_metrics_time.json', senc.cuda().eval(), sdec.cuda().eval(),
                            INSTRUCTION_LEN, max_episode_len=EPISODE_LEN)
random.setstate(state)
spk.store = features.FeatureStore(synth.feature_table(21, n_rows))
spk.sweep_test_after = 0
knows_switch = 'caption_metrics' in inspect.signature(se.SpeakerEvaluation.__init__).parameters
assert knows_switch or off_only, 'this checkout has no caption metrics: --off-only'
ev_off = se.SpeakerEvaluation(env=env)
data0, state0 = list(env.data), random.getstate()


def rewind():
    env.data[:] = data0
    random.setstate(state0)


def sweep_off():
    return ev_off.score_speaker(spk)[0]


fns = [sweep_off]
names = {sweep_off: 'score_speaker, caption metrics off'}
if not off_only:
    ev_on = se.SpeakerEvaluation(env=env, caption_metrics=True)
    ev_host = se.SpeakerEvaluation(env=env, device='cpu', caption_metrics=True)
    rewind()
    kept = dict(spk.test(use_dropout=False, feedback='argmax'))

    def sweep_on():
        return ev_on.score_speaker(spk)[0]

    def results_host():
        return ev_host.score_results(kept)[0]

    def results_device():
        return ev_on.score_results(kept)[0]

    fns += [sweep_on, results_host, results_device]
    names.update({sweep_on: 'score_speaker, caption metrics on (one sweep, one host sync)',
                  results_host: 'score_results on kept results, caption metrics on, on the host',
                  results_device: 'score_results on kept results, caption metrics on, on the device'})

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
assert ev_off.fallbacks == 0 and ev_off.last_host_syncs == 1
for fn in fns:
    ms = [x * 1e3 for x in times[fn]]
    say('%s: %-66s median %.2f ms  min %.2f  max %.2f  (%d runs, %d instructions, %d minibatches of %d, %d words)'
        % (label, names[fn], statistics.median(ms), min(ms), max(ms), REPS, len(items), len(spk.losses), BATCH,
           INSTRUCTION_LEN))
if not off_only:
    assert ev_on.fallbacks == 0 and ev_on.last_host_syncs == 1 and ev_on.captions['on_host'] == []
    assert all(last[sweep_on][k] == last[sweep_off][k] for k in last[sweep_off])
    host, dev = ev_host.captions, ev_on.captions
    assert host['rouge_l'] == dev['rouge_l'] and last[sweep_on]['rouge_l'] == last[results_host]['rouge_l']
    worst = max(abs(host['cider_d'][p] - dev['cider_d'][p]) for p in host['cider_d'])
    worst_part = max(abs(a - b) for p in host['parts'] for k in ('dot', 'hnorm2')
                     for a, b in zip(np.ravel(host['parts'][p][k]), np.ravel(dev['parts'][p][k])))
    say('summary with the switch on: %s' % last[sweep_on])
    say('device against host over %d paths: rouge_l equal; largest |cider_d difference| %.3g, largest |dot or hnorm2 '
        'difference| %.3g (largest hnorm2 %.1f); corpus cider_d differs by %.3g'
        % (len(host['cider_d']), worst, worst_part, max(max(host['parts'][p]['hnorm2']) for p in host['parts']),
           abs(last[results_host]['cider_d'] - last[results_device]['cider_d'])))
if out_path:
    with open(out_path, 'a' if '--append' in sys.argv else 'w') as f:
        f.write('\n'.join(lines) + '\n')
