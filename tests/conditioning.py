"""Conditioning envelope of the att-feed speaker's logits (tests/test_conditioning_host.py, tests/test_gpu_grads_f64.py,
tests/test_gpu_module_ladder.py).  Importable without a GPU.

The float64 oracle (oracle/torch_ref.py) is run again with the result of every operator it composes rounded once to fp32
(`torch_ref.rounded`): to nearest, and `n_random` times with a seeded random relative perturbation within +-2^-24.  Each
such run is a perfect implementation that merely STORES its operator results in fp32; how far its logits land from the
plain float64 ones is a property of the case (its conditioning), not of any kernel.  Per (step, row)

    env[t, b]   = max over those runs of max_v |logit_k[t, b, v] - logit_f64[t, b, v]|
    bound[t, b] = max(1e-4, K * env[t, b])                 K = tests/grad_compare.K

replaces the single fp32 evaluation of the reference as the yardstick: that one is one draw from the same distribution,
and which draw depends on the BLAS summation order, i.e. on the host and its thread count (see
tests/test_conditioning_host.py).  The envelope is deterministic: one generator, seeded once, drawn from in a fixed order.
"""
import functools

import numpy as np
import torch

from oracle import np_env, rng as orng, torch_ref
from speaker_follower_amd import synth
from tests import grad_compare as gc

N_RANDOM = 32            # the maximum over 8 trials still varied by 2x between seeds; 32 trials cost about 2 s
ENV_SEED = 1
ABS_BOUND = 1e-4         # the suite's logit bound (tests/test_gpu_grads_f64.py)
WELL_CONDITIONED = 2.5e-5   # a row whose envelope stays below this keeps the plain 1e-4 bound (K * env <= 1e-4)

SEED = 4242                         # tests/test_gpu_grads_f64.py: the engines' dropout seed
SPK_ENC_SEED_XOR = 0x2545F491       # SpeakerEngine: encoder mask seed = seed ^ this


class S4:
    """The oracle's side of tests/test_gpu_grads_f64.py::_s4: att-feed speaker decoder, B 12, 10 words, seed 31, 48
    viewpoints, paths of 4-6 steps, module-level dropout sites (encoder 2t / 2Tp + 1, decoder 4t + k)."""
    B, S, WSEED, NVP = 12, 10, 31, 48

    def __init__(self, train):
        d = synth.FULL
        self.train, self.dims = train, d
        self.senc_w, _ = synth.speaker_weights(self.WSEED, d)
        self.sdec_w = synth.speaker_decoder_att_feed_weights(self.WSEED, d)
        self.sb = synth.speaker_batch(seed=self.WSEED + 1, batch=self.B, n_viewpoints=self.NVP, min_len=4, max_len=9, dims=d)
        self.table = synth.feature_table(self.WSEED + 2, self.NVP)
        self.acts, self.feats, self.path_mask = np_env.dense_speaker_inputs(self.sb, self.table,
                                                                            np_env.static_loc_embeddings())
        self.instr_seq, _, _ = np_env.batch_instructions_from_encoded(self.sb.instr, 80)
        self.Tp = len(self.acts)
        self.rows = np.arange(self.B)
        self._w = {}

    def enc_drop(self, t):
        se, H, F, Tp = SEED ^ SPK_ENC_SEED_XOR, self.dims.hidden, self.dims.feat, self.Tp
        if t == 'ctx':
            return torch.tensor(orng.dropout_mask(se, 2 * Tp + 1, self.rows, Tp * H, 0.5).reshape(self.B, Tp, H))
        return torch.tensor(orng.dropout_mask(se, 2 * t, self.rows, 2 * F, 0.5))

    def dec_drop(self, t):
        H = self.dims.hidden
        return (None,) + tuple(torch.tensor(orng.dropout_mask(SEED, 4 * t + k, self.rows, n, 0.5))
                               for k, n in ((1, H), (2, H), (3, 2 * H)))

    def weights(self, dtype):
        if dtype not in self._w:
            self._w[dtype] = (torch_ref.to_torch(self.senc_w, dtype=dtype),
                              torch_ref.to_torch(self.sdec_w, dtype=dtype))
        return self._w[dtype]

    def run(self, tape=None, dtype=torch.float64):
        """The logits of every word step ([S] x [B, vocab]) under whatever rounding is in force."""
        e, d = self.weights(dtype)
        with torch.no_grad():
            res = torch_ref.speaker_score(e, d, self.acts, self.feats, torch.tensor(self.path_mask),
                                          torch.tensor(self.instr_seq), self.S, 'teacher',
                                          enc_drop=self.enc_drop if self.train else None,
                                          dec_drop=self.dec_drop if self.train else None, tape=tape)
        return res['logits']


def _dist(a, b):
    """max over the trailing axes of |a - b| where b is finite: [rows]."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    d = np.where(np.isfinite(b), np.abs(a - np.where(np.isfinite(b), b, 0.0)), 0.0)
    return d.reshape(d.shape[0], -1).max(1)


def logit_distance(got, ref):
    """[steps, rows]: max_v |got - ref| of every (step, row), finite reference entries."""
    return np.stack([_dist(g.detach().numpy() if hasattr(g, 'detach') else g,
                           r.detach().numpy() if hasattr(r, 'detach') else r) for g, r in zip(got, ref)])


def tape_entries(tape):
    """{(part, name): [steps] x tensor [rows, ...]} of a `speaker_score` tape; the encoder's context ([B, Tp, H]) is read
    as one entry per path step."""
    out = {}
    for part, sub in tape.items():
        for name, v in sub.items():
            if isinstance(v, list):
                out[(part, name)] = v
            elif v.dim() == 3:
                out[(part, name)] = [v[:, t] for t in range(v.shape[1])]
            else:
                out[(part, name)] = [v]
    return out


def tape_distance(got, ref):
    """{(part, name): [steps, rows]} -- `logit_distance` for every tape entry of `ref` (entries of tape_entries())."""
    return {k: np.stack([_dist(g.numpy(), r.numpy()) for g, r in zip(got[k], ref[k])]) for k in ref}


def envelope(run, n_random=N_RANDOM, seed=ENV_SEED, tape_env=None):
    """run(tape=None) -> the logits of every step, evaluated under the rounding in force.  Returns env [steps, rows]: the
    maximum over the nearest-rounded run and `n_random` randomly rounded runs (one generator seeded with `seed`) of
    max_v |logit_k - logit_f64|.  tape_env: a dict that receives the same maximum for every tape entry,
    {(part, name): [steps, rows]}, and under the key 'f64' the plain float64 tape's entries."""
    want_tape = tape_env is not None
    t64 = {} if want_tape else None
    ref = run(t64)
    if want_tape:
        t64 = tape_entries(t64)
    gen = torch.Generator().manual_seed(seed)
    env, tenv = None, {}
    for k in range(n_random + 1):
        tp = {} if want_tape else None
        with torch_ref.rounded('nearest' if k == 0 else 'random', None if k == 0 else gen):
            got = run(tp)
        d = logit_distance(got, ref)
        env = d if env is None else np.maximum(env, d)
        if want_tape:
            for key, dist in tape_distance(tape_entries(tp), t64).items():
                tenv[key] = np.maximum(tenv[key], dist) if key in tenv else dist
    if want_tape:
        tape_env.update(tenv)
        tape_env['f64'] = t64
    return env


def entry_bounds(env):
    """The per-(step, row) logit bound: max(1e-4, K * env)."""
    return np.maximum(ABS_BOUND, gc.K * np.asarray(env))


@functools.lru_cache(maxsize=None)
def s4(train):
    return S4(train)


@functools.lru_cache(maxsize=None)
def s4_envelope(train):
    """(env [steps, rows], tape_env) of the S4 case, computed once per process and shared (read-only) by every test that
    needs it."""
    tape_env = {}
    env = envelope(s4(train).run, tape_env=tape_env)
    for v in [env] + [v for k, v in tape_env.items() if k != 'f64']:
        v.setflags(write=False)
    return env, tape_env
