"""The speaker's decoding pass at the reference's trainval vocabulary (1 086 words: outside the persistent word loop, so
every pass is sf_speaker_words_fwd: about five launches per word), B = 100 paths, S = 80 words, in ONE process after a
warm-up:

  * the per-step `argmax` pass against the `sample` pass of SpeakerEngine.wide_sample (speaker_glue_wide_sample_kernel),
    issued eagerly and as a replayed hipGraph: median / min / max of BLOCKS timed blocks of PASSES passes each, the two
    feedbacks interleaved block by block (a host clock around work that ends in a device synchronise);
  * the glue launch alone (sf_speaker_glue_fwd on [B,1086] logits), feedback 1 against feedback 2, from the library's own
    launch events (kernel_profile).

On a tree without the switch (the commit before it) the `sample` legs are left out and only the argmax figures are
printed: that is the base the sampled pass is compared with.  Prints one JSON line at the end.
    python tools/speaker_wide_sample_time.py [--blocks 12] [--passes 10]
"""
import argparse
import ctypes as C
import dataclasses
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from speaker_follower_amd import synth, features, model, speaker, _lib   # noqa: E402
from speaker_follower_amd._lib import kernel_profile                      # noqa: E402
from speaker_follower_amd.runtime import ptr, stream                      # noqa: E402

VOCAB, PAD, EOS = 1086, 0, 2


def spread(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), n=len(xs))


def glue_alone(B, feedback, launches=200):
    g = np.random.default_rng(7)
    ldv = (VOCAB + 3) & ~3
    lg = torch.zeros(B, ldv, device='cuda')
    lg[:, :VOCAB] = torch.from_numpy((g.standard_normal((B, VOCAB)) * 1.5).astype(np.float32)).cuda()
    target = torch.from_numpy(g.integers(0, VOCAB, B)).cuda()
    w = torch.empty(B, dtype=torch.int64, device='cuda')
    score, nll, live = (torch.empty(B, device='cuda') for _ in range(3))
    ended = torch.zeros(B, dtype=torch.uint8, device='cuda')

    def launch(t):
        smp = C.byref(_lib.Sample(99, t, 0)) if feedback == 2 else None
        _lib.call('sf_speaker_glue_fwd', B, VOCAB, ldv, ptr(lg), ptr(target), feedback, PAD, EOS, ptr(ended), ptr(w),
                  ptr(score), ptr(nll), ptr(live), smp, stream())
    for t in range(20):
        launch(t)
    torch.cuda.synchronize()
    with kernel_profile() as prof:
        for t in range(launches):
            launch(t)
        torch.cuda.synchronize()
    return {k: dict(calls=v['calls'], avg_us=v['avg_us'], min_us=v['min_us'], max_us=v['max_us']) for k, v in prof.rows.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--blocks', type=int, default=12)
    ap.add_argument('--passes', type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('speaker_wide_sample_time.py measures on a GPU: none found')
    torch.cuda.set_device(0)
    B, S, NVP = 100, 80, 128
    wide = hasattr(speaker, 'check_sample_vocab')
    legs = ('argmax', 'sample') if wide else ('argmax',)
    d = dataclasses.replace(synth.FULL, vocab=VOCAB)
    senc_w, sdec_w = synth.speaker_weights_peaky(31, d)
    enc = model.SpeakerEncoderLSTM(d.feat, d.feat, d.hidden, 0.5)
    dec = model.SpeakerDecoderLSTM(d.vocab, d.word, d.hidden, 0.5, glove=sdec_w['embedding.weight'])
    enc.load_state_dict({k: torch.tensor(v) for k, v in senc_w.items()})
    dec.load_state_dict({k: torch.tensor(v) for k, v in sdec_w.items()})
    enc.cuda().eval()
    dec.cuda().eval()
    store = features.FeatureStore(synth.feature_table(7, NVP))
    batch = speaker.DeviceSpeakerBatch.from_synth(synth.speaker_batch(seed=9, batch=B, n_viewpoints=NVP, dims=d))

    def engine():
        eng = speaker.SpeakerEngine(enc, dec, store)
        eng.dropout_seed = 0x1234
        if wide:
            eng.wide_sample = True
        return eng
    eager = {m: engine() for m in legs}
    graphs = {m: engine().capture(batch, S, m) for m in legs}
    for m in legs:
        assert not graphs[m][1].persistent                                # 1 086 words: the per-step kernels
    times = {(how, m): [] for how in ('eager', 'graph') for m in legs}
    with torch.no_grad():
        for blk in range(args.blocks + 2):
            for m in legs:
                for how, run in (('eager', lambda: eager[m].score(batch, S, m, train=False)), ('graph', graphs[m][0])):
                    for _ in range(2):
                        run()
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(args.passes):
                        run()
                    torch.cuda.synchronize()
                    if blk >= 2:                                          # (warm-up: code objects, caches, clocks)
                        times[(how, m)].append(1e3 * (time.perf_counter() - t0) / args.passes)
    passes = {'%s_%s' % k: spread(v) for k, v in times.items()}
    for k, t in sorted(passes.items()):
        print('pass B=%d x %d words, vocab %d, %-12s median %.3f  min %.3f  max %.3f ms (n = %d)'
              % (B, S, VOCAB, k + ':', t['median'], t['min'], t['max'], t['n']))
    glue = {'feedback_%d' % f: glue_alone(B, f) for f in ((1, 2) if wide else (1,))}
    for f, rows in sorted(glue.items()):
        for k, v in sorted(rows.items()):
            print('glue alone, %s: %-50s %4d launches, %7.2f us each (min %.2f, max %.2f)'
                  % (f, k[:50], v['calls'], v['avg_us'], v['min_us'], v['max_us']))
    print(json.dumps(dict(wide_sample=wide, pass_ms=passes, glue_us=glue)))


if __name__ == '__main__':
    main()
