"""Bidirectional encoder (train.py --bidirectional: hidden 256 x 2 directions, GloVe) on the MI355X:
  * the encoder alone at B = 100, T = 80 (eval, no autograd): both directions as ONE persistent launch
    (sf_encoder_bilstm_fwd, enc_persist_kernel<2>) against the per-step kernels of the same entry (enc.persistent =
    False), and the unidirectional hidden-512 encoder (one persistent launch) for scale;
  * one training iteration at the follower's configs[1] shape (batch 100, 20 steps, 10 567 viewpoints, student forcing,
    dropout on, BPTT, two Adam steps) with a bidirectional encoder: eager vs replayed (bench.measure_train).
Prints one JSON object.  python tools/bidir_time.py [--iters N] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def bidir_models(dev, enc_seed=19, dec_seed=101):
    from speaker_follower_amd import model, synth
    d = synth.FULL
    w = synth.bidirectional_encoder_weights(enc_seed)
    enc = model.EncoderLSTM(d.vocab, d.word, d.hidden // 2, 0, 0.5, bidirectional=True, glove=w['embedding.weight'])
    enc.load_state_dict({k: torch.tensor(v) for k, v in w.items()})
    _, dec_w = synth.follower_weights_peaky(dec_seed)
    dec = model.AttnDecoderLSTM(d.feat, d.hidden, 0.5, feature_size=d.feat)
    dec.load_state_dict({k: torch.tensor(v) for k, v in dec_w.items()})
    return enc.to(dev), dec.to(dev)


def time_calls(fn, iters, warmup=5):
    """Milliseconds per call: device events around `iters` back-to-back calls, behind `warmup` untimed ones."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def encoder_alone(dev, iters, rounds=3):
    from speaker_follower_amd import synth
    import bench
    B, T = 100, 80
    r = np.random.default_rng(0)
    lens = [int(x) for x in r.integers(10, T + 1, size=B)]
    lens[0] = T
    seq = np.zeros((B, T), np.int64)
    for b, n in enumerate(lens):
        seq[b, :n] = r.integers(4, synth.FULL.vocab, size=n)
    seq = torch.tensor(seq, device=dev)
    enc, _ = bidir_models(dev)
    enc.eval()
    uni, _, _, _ = bench.build_models(101, dev)
    uni.eval()
    res = {'persistent': [], 'per_step': [], 'unidirectional_512': []}
    paths = {}
    with torch.no_grad():
        for _ in range(rounds):                               # alternated: the spread of each is visible
            for key, persistent in (('persistent', True), ('per_step', False)):
                enc.persistent = persistent
                res[key].append(time_calls(lambda: enc(seq, lens), iters))
                paths[key] = enc.last_path
            res['unidirectional_512'].append(time_calls(lambda: uni(seq, lens), iters))
    enc.persistent = True
    out = {k: dict(ms_median=float(np.median(v)), ms_all=[round(x, 4) for x in v]) for k, v in res.items()}
    out['paths'] = paths
    out['us_per_step_persistent'] = 1e3 * out['persistent']['ms_median'] / T
    out['shape'] = dict(B=B, T=T, hidden_per_direction=256)
    return out


def train_iteration(dev, iters):
    import bench
    from speaker_follower_amd import features, follower, synth
    enc, dec = bidir_models(dev)
    store = features.FeatureStore(bench.device_table(10567, 1234, dev), device=dev)
    fb = synth.follower_batch(seed=0, batch=100, steps=20, n_viewpoints=10567)
    batch = follower.DeviceFollowerBatch.from_synth(fb, device=dev)
    t = bench.measure_train(enc, dec, store, batch, 20, iters, 5)
    return dict(eager_ms=t['eager']['ms_per_iteration'], replay_ms=t['ms_per_iteration'], loss=t['loss'],
                encoder_path=getattr(enc, 'last_path', None), encoder_backward_path=getattr(enc, 'last_backward_path', None))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bidir_time.py needs a GPU')
    sys.argv = ['bench.py']                                   # (bench parses its own arguments at import)
    dev = torch.device('cuda', 0)
    out = dict(encoder=encoder_alone(dev, args.iters), train_iteration=train_iteration(dev, max(10, args.iters // 2)))
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
