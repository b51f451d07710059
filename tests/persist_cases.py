"""Shapes, inputs and float64 models for tests/test_gpu_persistent_edges.py (checked on the host by
tests/test_persist_cases_host.py): the persistent launches of csrc/sf_persist.hip -- the speaker's word loop
(spk_persist_kernel), the encoder's recurrence (enc_persist_kernel<1|2>) and its backward (enc_bwd_persist_kernel<1|2>)
-- one launch at a time, at every edge of their hand-built partition: 8 row groups x 32 workgroups x 16 rows, three
rotating sentinel buffers, 32 vocabulary columns per workgroup, one lane per path step.

The models are built on oracle/torch_ref.py and run in the dtype they are asked for: float64 is the reference, the
float32 evaluation of the SAME model on the same inputs is the yardstick e32.  The word loop's model is teacher-forced
on the words the launch emitted, so one flipped near-tie cannot cascade: every step is compared on its own.

The comparison rule is the project's (tests/grad_compare.py): per tensor e = max|gpu - r64| / max|r64|, e32 likewise for
the float32 model, and e <= max(K e32, FLOOR), e <= CEILING."""
import dataclasses
import functools
from collections import namedtuple

import numpy as np
import torch

from oracle import torch_ref
from speaker_follower_amd import synth
from tests.grad_compare import CEILING, FLOOR, K

PAD, EOS, BOS = synth.PAD, synth.EOS, synth.BOS

# ------------------------------------------------------------------------------------------ constants
# (speaker_follower_amd/csrc/sf_persist.hip; the line each value mirrors)
EP_GROUPS = 8                                 # :41   row groups (= XCDs)
EP_SLOTS = 32                                 # :42   workgroups per group, 16 hidden units each
EP_ROWS = 16                                  # :43   rows per group
EP_TMAX = 128                                 # :44   steps of the encoder launches (s_tok[16][128], :172)
SP_TPMAX = 12                                 # :655  path steps of the word loop (one lane each)
N_BUFFERS = 3                                 # :812  bo = (t % 3) * SPX_BUF
SLOT_UNITS = 16                               # :42, :757  ej = 16 * slot + eu
VOC_COLS = 32                                 # :770  col0 = 32 * slot + eu, col1 = col0 + 16
VOCAB_MIN, VOCAB_MAX = 32, VOC_COLS * EP_SLOTS        # :1249-1250  speaker_persistent_supported
B_MAX = EP_GROUPS * EP_ROWS                   # :1169, :1249
H = SLOT_UNITS * EP_SLOTS                     # :1169, :1249  H == 16 * EP_SLOTS
H_BI = SLOT_UNITS * (EP_SLOTS // 2)           # :1203  per direction of the two-direction launch
E = synth.FULL.word

SPK_KERNEL, SPK_SAMPLE_KERNEL = 'spk_persist_kernel', 'spk_persist_kernel<sample>'           # :1276-1278
ENC_KERNEL, ENC_BI_KERNEL = 'enc_persist_kernel', 'enc_persist_kernel<bidir>'                # :1189, :1224
ENC_BWD_KERNEL, ENC_BWD_BI_KERNEL = 'enc_bwd_persist_kernel', 'enc_bwd_persist_kernel<bidir>'   # :1297, :1243


def ldv(vocab):
    """Row stride of the logits tape (sf_api_speaker.hip: spk_ldv)."""
    return (vocab + 3) & ~3


def rpg(B):
    """Rows per group (:1181, :1266  `a.rpg = ceil_div(B, EP_GROUPS)`)."""
    return -(-B // EP_GROUPS)


def group_rows(B):
    """Rows of each of the 8 groups (:729-730  row0 = grp * rpg, nrows = max(0, min(rpg, B - row0)))."""
    return [max(0, min(rpg(B), B - g * rpg(B))) for g in range(EP_GROUPS)]


def vocab_slots(vocab):
    """(full slots, columns of the partly filled slot, empty slots) of the 32 vocabulary workgroups."""
    full, part = divmod(vocab, VOC_COLS)
    return full, part, EP_SLOTS - full - (1 if part else 0)


def last_slot_first(vocab):
    """First column of the last slot that holds a column."""
    return VOC_COLS * ((vocab - 1) // VOC_COLS)


def speaker_supported(B, Tp, vocab):
    """speaker_persistent_supported (:1248-1251) at H = 512 on a device with >= 256 CUs."""
    return 1 <= B <= B_MAX and 1 <= Tp <= SP_TPMAX and VOCAB_MIN <= vocab <= VOCAB_MAX


def encoder_supported(B, T):
    """encoder_persistent_supported (:1168-1171) at H = 512 (two directions: 256 each, :1202-1205)."""
    return 1 <= B <= B_MAX and 1 <= T <= EP_TMAX


# ---------------------------------------------------------------------------------------------- cases
Spk = namedtuple('Spk', 'vocab Tp B S mask peaky')          # mask: True = the ragged path mask, False = ctx_mask NULL
Enc = namedtuple('Enc', 'B T Lpad')
Teacher = namedtuple('Teacher', 'B S vocab Tp')
EncBwd = namedtuple('EncBwd', 'B T train bidir')
Refusal = namedtuple('Refusal', 'what status vocab Tp B feedback sample')

SPK_DEFAULT = dict(vocab=935, Tp=3, B=9, S=4, mask=True, peaky=False)      # 935: sub_train_vocab.txt, 29 slots + 7 columns


def _spk(**kw):
    return Spk(**dict(SPK_DEFAULT, **kw))


VOCABS = (32, 33, 63, 64, 65,          # one slot; the second slot holding one column
          479, 480, 481,               # at 480 and below slots 15 and 31 are both empty: a lane of the merge holds two
          512, 513,                    # at 512 every second-half slot is empty
          935, 991,                    # the live vocabularies
          1023, 1024)                  # the last slot at 31 and at 32 columns
TPS = (1, 2, SP_TPMAX - 1, SP_TPMAX)
BS = (1, EP_GROUPS, EP_GROUPS + 1, 2 * EP_GROUPS, 2 * EP_GROUPS + 1, B_MAX - EP_GROUPS, B_MAX - EP_GROUPS + 1, B_MAX)
STEPS = (1, 2, 3, 4, 7)
SPEAKER = ([_spk(vocab=v) for v in VOCABS] +
           [_spk(Tp=tp, mask=m) for tp in TPS for m in (False, True)] +
           [_spk(B=b) for b in BS] +
           [_spk(S=s) for s in STEPS] +
           [_spk(vocab=v, peaky=True) for v in (33, 935, 1024)] + [_spk(Tp=SP_TPMAX, peaky=True), _spk(B=B_MAX - 7, peaky=True)])
FEEDBACKS = ('teacher', 'argmax')

# two columns with identical decoder2action rows and biases (vocab, (lower, higher)): what the pair reaches
TIES = [(1024, (100, 116)),            # one thread's two columns (col0, col0 + 16)
        (1024, (100, 101)),            # two lanes of one workgroup
        (1024, (100, 132)),            # neighbouring workgroups
        (1024, (100, 612)),            # slots s and s + 16, merged inside one lane
        (935, (40, 934))]              # an early column against the last column of the partly filled slot
TIE_B, TIE_S = 9, 3

SAMPLE_VOCABS = (32, 33, 480, 935, 1024)

REFUSALS = [Refusal('vocab = VOCAB_MIN - 1', 2, VOCAB_MIN - 1, 3, 9, 1, False),
            Refusal('vocab = VOCAB_MAX + 1', 2, VOCAB_MAX + 1, 3, 9, 1, False),
            Refusal('Tp = SP_TPMAX + 1', 2, 935, SP_TPMAX + 1, 9, 1, False),
            Refusal('B = B_MAX + 1', 2, 935, 3, B_MAX + 1, 1, False),
            Refusal('feedback 2 without sample', 1, 935, 3, 9, 2, False)]

ENCODER = [Enc(1, 1, 1), Enc(9, 1, 80), Enc(9, 2, 80), Enc(9, 3, 80), Enc(17, 4, 4), Enc(9, 80, 80),
           Enc(9, EP_TMAX - 1, EP_TMAX), Enc(17, EP_TMAX, EP_TMAX), Enc(B_MAX - 7, EP_TMAX, EP_TMAX), Enc(B_MAX, 5, 80),
           Enc(B_MAX - EP_GROUPS, 5, 80)]
ENCODER_FALLBACK = Enc(9, EP_TMAX + 1, EP_TMAX + 1)
TEACHER = [Teacher(1, 1, 33, 1), Teacher(9, 2, 935, SP_TPMAX), Teacher(17, 4, 1024, 3)]
ENCODER_BWD = [EncBwd(1, 1, False, False), EncBwd(9, 2, False, False), EncBwd(9, EP_TMAX, True, False),
               EncBwd(B_MAX - 7, 7, False, False), EncBwd(B_MAX, 3, True, False),
               EncBwd(1, 1, False, True), EncBwd(9, EP_TMAX, False, True)]


def boundaries():
    """Every boundary of the partition as (name, table, field, value below, value above), derived from the constants
    alone; `above` None: the far side is a refusal (an entry of REFUSALS with a larger / smaller value of the field) or,
    for the encoder's T, the fall-back case ENCODER_FALLBACK."""
    out = [('one vocabulary slot | a second slot holding one column', SPEAKER, 'vocab', VOC_COLS, VOC_COLS + 1),
           ('two vocabulary slots | a third', SPEAKER, 'vocab', 2 * VOC_COLS, 2 * VOC_COLS + 1),
           ('second slot at 31 | 32 columns', SPEAKER, 'vocab', 2 * VOC_COLS - 1, 2 * VOC_COLS),
           ('slots 15 and 31 both empty | slot 15 holds a column', SPEAKER, 'vocab', VOC_COLS * (EP_SLOTS // 2 - 1),
            VOC_COLS * (EP_SLOTS // 2 - 1) + 1),
           ('slot 14 at 31 | 32 columns', SPEAKER, 'vocab', VOC_COLS * (EP_SLOTS // 2 - 1) - 1, VOC_COLS * (EP_SLOTS // 2 - 1)),
           ('every second-half slot empty | slot 16 holds a column', SPEAKER, 'vocab', VOC_COLS * EP_SLOTS // 2,
            VOC_COLS * EP_SLOTS // 2 + 1),
           ('last slot at 31 | 32 columns', SPEAKER, 'vocab', VOCAB_MAX - 1, VOCAB_MAX),
           ('smallest vocabulary', SPEAKER, 'vocab', VOCAB_MIN, None), ('largest vocabulary', SPEAKER, 'vocab', VOCAB_MAX, None),
           ('one path step | two', SPEAKER, 'Tp', 1, 2), ('lane 11 idle | live', SPEAKER, 'Tp', SP_TPMAX - 1, SP_TPMAX),
           ('most path steps', SPEAKER, 'Tp', SP_TPMAX, None),
           ('one row | one row in every group', SPEAKER, 'B', 1, EP_GROUPS),
           ('rpg 1 | rpg 2 with a one-row group and three empty ones', SPEAKER, 'B', EP_GROUPS, EP_GROUPS + 1),
           ('rpg 2 full | rpg 3 with a ragged last group', SPEAKER, 'B', 2 * EP_GROUPS, 2 * EP_GROUPS + 1),
           ('rpg 15 | rpg 16 with a ragged last group', SPEAKER, 'B', B_MAX - EP_GROUPS, B_MAX - EP_GROUPS + 1),
           ('last group ragged | full', SPEAKER, 'B', B_MAX - 7, B_MAX), ('most rows', SPEAKER, 'B', B_MAX, None),
           ('most encoder steps', ENCODER, 'T', EP_TMAX, None), ('s_tok row nearly full | full', ENCODER, 'T', EP_TMAX - 1, EP_TMAX),
           ('encoder: rpg 2 | rpg 3', ENCODER, 'B', EP_GROUPS + 1, 2 * EP_GROUPS + 1),
           ('encoder: rpg 15 | rpg 16', ENCODER, 'B', B_MAX - EP_GROUPS, B_MAX - 7),
           ('encoder: last group ragged | full', ENCODER, 'B', B_MAX - 7, B_MAX)]
    # the buffer rotation from its start: every step count up to one whole turn, one past it, and two turns past
    for s in range(1, N_BUFFERS + 1):
        out.append(('word loop: %d step(s) | %d' % (s, s + 1), SPEAKER, 'S', s, s + 1))
        out.append(('encoder: %d step(s) | %d' % (s, s + 1), ENCODER, 'T', s, s + 1))
    out.append(('word loop: two turns of the buffers and one step', SPEAKER, 'S', 2 * N_BUFFERS + 1, 2 * N_BUFFERS + 1))
    return out


# --------------------------------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=4)
def speaker_decoder_weights(vocab, peaky=False, seed=404):
    """The decoder state (numpy, keyed like SpeakerDecoderLSTM's state_dict) for any vocabulary."""
    dims = dataclasses.replace(synth.FULL, vocab=vocab)
    return (synth.speaker_weights_peaky if peaky else synth.speaker_weights)(seed, dims)[1]


def tie_weights(dec, pair, bias=20.0):
    """`dec` with identical decoder2action rows and biases in the two columns of `pair`, both the clear maximum."""
    lo, hi = pair
    out = dict(dec)
    w, b = dec['decoder2action.weight'].copy(), dec['decoder2action.bias'].copy()
    w[hi] = w[lo]
    b[lo] = b[hi] = np.float32(bias)
    out['decoder2action.weight'], out['decoder2action.bias'] = w, b
    return out


def path_mask(B, Tp):
    """uint8 [B, Tp], 1 = padded path step: row 0 of full length Tp, row 1 of length 1, the rest anywhere between."""
    lens = [Tp, 1] + [1 + (5 * b + 2) % Tp for b in range(2, B)]
    m = np.zeros((B, Tp), np.uint8)
    for b in range(B):
        m[b, lens[b]:] = 1
    return m


def special_columns(vocab):
    """Columns the targets must reach: the last one, the first of the last slot that holds any, EOS, and both sides of
    the first slot edge (column 0 is PAD: every tail reaches it)."""
    return [vocab - 1, last_slot_first(vocab), EOS, min(VOC_COLS, vocab) - 1, min(VOC_COLS, vocab - 1)]


def speaker_targets(rng, vocab, S, B):
    """int64 [S, B]: row 0 live at every step, row B - 1 (B >= 3) all PAD, the others live for 1 .. S steps with a PAD
    tail; the live cells hold random words >= 4 and, in step-major order, `special_columns`."""
    n = [S] + [1 + (3 * b) % S for b in range(1, B)]
    if B >= 3:
        n[B - 1] = 0
    t = np.full((S, B), PAD, np.int64)
    cells = [(s, b) for s in range(S) for b in range(B) if s < n[b]]
    for s, b in cells:
        t[s, b] = rng.integers(4, vocab)
    for (s, b), col in zip(cells, [c for c in special_columns(vocab) if c != PAD]):      # (vocab 32: the slot begins at PAD)
        t[s, b] = col
    return t


SpkInputs = namedtuple('SpkInputs', 'ctx h_init c_init mask targets')


def speaker_inputs(case, seed=0):
    """ctx [B, Tp, H], h_init, c_init [B, H] in tanh range (what the speaker's encoder hands over; padded path steps
    hold encoder outputs too, not zeros: only the mask hides them), the path mask and the targets."""
    rng = np.random.default_rng([seed, case.vocab, case.Tp, case.B, case.S, 41])
    f32 = np.float32
    ctx = np.tanh(rng.standard_normal((case.B, case.Tp, H))).astype(f32)
    h_init = np.tanh(0.5 * rng.standard_normal((case.B, H))).astype(f32)
    c_init = (0.5 * rng.standard_normal((case.B, H))).astype(f32)
    mask = path_mask(case.B, case.Tp) if case.mask else None
    return SpkInputs(ctx, h_init, c_init, mask, speaker_targets(rng, case.vocab, case.S, case.B))


def encoder_tokens(B, T, Lpad, seed=0, vocab=synth.FULL.vocab):
    """(seq int64 [B, Lpad], lens): row 0 of full length T, the last row (B > 1) of one token, the rest anywhere between;
    PAD behind each length."""
    rng = np.random.default_rng([seed, B, T, Lpad, 43])
    lens = [int(x) for x in rng.integers(1, T + 1, size=B)]
    lens[0] = T
    if B > 1:
        lens[-1] = 1
    seq = np.zeros((B, Lpad), np.int64)
    for b, n in enumerate(lens):
        seq[b, :n] = rng.integers(4, vocab, size=n)
    return seq, lens


# --------------------------------------------------------------------------------------------- models
def _t(a, dtype):
    return torch.as_tensor(np.asarray(a)).to(dtype)


def _np64(t):
    return t.detach().double().numpy()


def word_stats(logits, words, targets, lse_cols=None):
    """The glue of every step (speaker.py:163-191) on logits [S, B, vocab] (a torch tensor; computed in its dtype):
    step_scores = log p(words[t + 1]) (0 for PAD), nll_term = -log p(target) (0 for PAD), live, ended.  lse_cols: the
    log-sum-exp over the first `lse_cols` columns only (a corruption the host test feeds the comparator)."""
    words, targets = torch.as_tensor(words), torch.as_tensor(targets)
    lse = torch.logsumexp(logits if lse_cols is None else logits[..., :lse_cols], dim=2)
    fed = words[1:]
    zero = torch.zeros((), dtype=logits.dtype)
    lw = logits.gather(2, fed[..., None])[..., 0] - lse
    lt = logits.gather(2, targets[..., None])[..., 0] - lse
    return dict(step_scores=_np64(torch.where(fed != PAD, lw, zero)), nll_term=_np64(torch.where(targets != PAD, -lt, zero)),
                live=(targets != PAD).numpy().astype(np.float32), ended=(fed == EOS).any(0).numpy().astype(np.uint8))


TENSORS = ('logits', 'alpha', 'h1', 'c1', 'step_scores', 'nll_term')      # compared under the rule; live / ended exactly


def word_loop(dec, inp, words, dtype=torch.float64, mask='own', lse_cols=None):
    """The word loop's own function (speaker.py:158-197 over torch_ref.speaker_decoder_step, eval mode), fed
    words[t] at step t: logits [S, B, vocab], alpha [S, B, Tp], h1 / c1 [S, B, H] and `word_stats` of them against
    inp.targets, all float64 numpy whatever the dtype of the evaluation."""
    w = torch_ref.to_torch(dec, dtype=dtype)
    mask = inp.mask if isinstance(mask, str) else mask
    m = None if mask is None else torch.as_tensor(np.asarray(mask).astype(bool))
    h, c, ctx = _t(inp.h_init, dtype), _t(inp.c_init, dtype), _t(inp.ctx, dtype)
    words = np.asarray(words)
    tape = dict(logits=[], alpha=[], h1=[], c1=[])
    with torch.no_grad():
        for t in range(words.shape[0] - 1):
            h, c, alpha, logit = torch_ref.speaker_decoder_step(w, torch.as_tensor(words[t]), h, c, ctx, m)
            for k, v in (('logits', logit), ('alpha', alpha), ('h1', h), ('c1', c)):
                tape[k].append(v)
        tape = {k: torch.stack(v) for k, v in tape.items()}
        out = word_stats(tape['logits'], words, inp.targets, lse_cols)
    out.update({k: _np64(v) for k, v in tape.items()})
    return out


def teacher_words(inp, B):
    """words [S + 1, B] of teacher feedback: <BOS>, then the targets."""
    return np.concatenate((np.full((1, B), BOS, np.int64), inp.targets), 0)


def argmax_rollout(dec, inp, dtype=torch.float64):
    """The word loop with argmax feedback run end to end in `dtype`: words [S + 1, B]."""
    w = torch_ref.to_torch(dec, dtype=dtype)
    m = None if inp.mask is None else torch.as_tensor(inp.mask.astype(bool))
    h, c, ctx = _t(inp.h_init, dtype), _t(inp.c_init, dtype), _t(inp.ctx, dtype)
    B = inp.h_init.shape[0]
    words = [torch.full((B,), BOS, dtype=torch.long)]
    with torch.no_grad():
        for _ in range(inp.targets.shape[0]):
            h, c, _, logit = torch_ref.speaker_decoder_step(w, words[-1], h, c, ctx, m)
            words.append(logit.argmax(1))
    return torch.stack(words).numpy()


def _direction(w, sfx, seq, lens, reverse, dtype, retain):
    """One direction of the packed nn.LSTM in the launch's STEP order (step t of the reverse direction of row b reads
    position len_b - 1 - t; a dead step t >= len_b reads position t and holds the state): the tapes hs, cs [T + 1, B, H],
    activated gates [T, B, 4H] (i, f, g, o), the pre-activation gates of every step (retain: with retained gradients), the
    direction's output [B, T, H] (zero beyond each length) and the final state."""
    seq = torch.as_tensor(np.asarray(seq))
    ln = torch.as_tensor(np.asarray(lens))
    B, T = seq.shape[0], int(ln.max())
    w_ih, w_hh = w['lstm.weight_ih_l0' + sfx], w['lstm.weight_hh_l0' + sfx]
    bias = w['lstm.bias_ih_l0' + sfx] + w['lstm.bias_hh_l0' + sfx]
    Hd = w_hh.shape[1]
    h = torch.zeros(B, Hd, dtype=dtype)
    c = torch.zeros(B, Hd, dtype=dtype)
    hs, cs, gates, pre, outs, poss = [h], [c], [], [], [], []
    rows = torch.arange(B)
    for t in range(T):
        live = t < ln
        pos = torch.where(live, ln - 1 - t, torch.full_like(ln, t)) if reverse else torch.full_like(ln, t)
        x = w['embedding.weight'][seq[rows, pos]]
        p = x @ w_ih.T + h @ w_hh.T + bias
        if retain:
            p.retain_grad()
        i, f, g, o = p.chunk(4, 1)
        i, f, g, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)
        c1 = f * c + i * g
        h1 = o * torch.tanh(c1)
        lv = live[:, None]
        h, c = torch.where(lv, h1, h), torch.where(lv, c1, c)
        hs.append(h)
        cs.append(c)
        gates.append(torch.cat((i, f, g, o), 1))
        pre.append(p)
        outs.append(torch.where(lv, h1, torch.zeros_like(h1)))
        poss.append(pos)
    ctx = torch.zeros(B, T, Hd, dtype=dtype).index_put((rows.repeat(T), torch.cat(poss)), torch.cat(outs))
    return dict(hs=torch.stack(hs), cs=torch.stack(cs), gates=torch.stack(gates), pre=pre, ctx=ctx, h=h, c=c)


def encoder_model(enc, seq, lens, drop_ctx=None, dtype=torch.float64, grad=False, shift=0):
    """EncoderLSTM.forward (model.py:81-104) with its tapes, for a state dict `enc` (numpy); a state holding the
    `_reverse` weights runs both directions (ctx = [forward | reverse], h_t = [h_reverse ; h_forward]).  Returns torch
    tensors: ctx (times drop_ctx when given), decoder_init, c_t and per direction ('f', 'r') the dict of `_direction`.
    grad: the weights require gradients and the pre-activation gates retain theirs.  shift: step t reads token t + shift
    (a corruption the host test feeds the comparator)."""
    w = torch_ref.to_torch(enc, requires_grad=grad, frozen=('embedding.weight',), dtype=dtype)
    seq = np.asarray(seq)
    if shift:
        seq = np.concatenate((seq[:, shift:], np.zeros((seq.shape[0], shift), seq.dtype)), 1)
    bidir = 'lstm.weight_ih_l0_reverse' in w
    with torch.set_grad_enabled(grad):
        f = _direction(w, '', seq, lens, False, dtype, grad)
        out = dict(w=w, f=f)
        if bidir:
            r = out['r'] = _direction(w, '_reverse', seq, lens, True, dtype, grad)
            ctx, h_t, c_t = torch.cat((f['ctx'], r['ctx']), 2), torch.cat((r['h'], f['h']), 1), torch.cat((r['c'], f['c']), 1)
        else:
            ctx, h_t, c_t = f['ctx'], f['h'], f['c']
        out['decoder_init'] = torch.tanh(h_t @ w['encoder2decoder.weight'].T + w['encoder2decoder.bias'])
        out['ctx'] = ctx if drop_ctx is None else ctx * _t(drop_ctx, dtype).reshape(ctx.shape)
        out['c_t'] = c_t
    return out


def _encoder_f64(enc, seq, lens):
    """The recurrence of an EncoderLSTM module in float64 on the host (model.py:81-104, eval mode): hs [T+1,B,H], cs."""
    w = {k: v.detach().cpu().numpy() for k, v in enc.state_dict().items()}
    f = encoder_model(w, seq.cpu().numpy(), lens)['f']
    return f['hs'], f['cs']


# ------------------------------------------------------------------------------------------ tolerance
def rel_err(got, ref64):
    """max |got - ref64| / max |ref64| (the tensor's own scale); a reference that is all zero admits only zero."""
    ref64 = np.asarray(ref64, np.float64)
    got = np.asarray(got, np.float64)
    assert got.shape == ref64.shape, (got.shape, ref64.shape)
    if got.size == 0:
        return 0.0
    d = float(np.abs(got - ref64).max()) if np.isfinite(got).all() else np.inf
    scale = float(np.abs(ref64).max())
    return d / scale if scale > 0 else (0.0 if d == 0 else np.inf)


def bound(e32):
    return min(max(K * e32, FLOOR), CEILING)


def compare(what, got, r64, r32, keys, named=None, rows=None):
    """Every tensor `keys` of `got` against the float64 model `r64` with the float32 model `r32` as yardstick: prints
    e and e32 per tensor, appends (what, key, e, e32, bound) to `rows`, raises AssertionError naming every tensor out of
    bound.  named: {key: bound} for a case whose own bound the module documents (never above CEILING)."""
    errors = []
    for k in keys:
        e, e32 = rel_err(got[k], r64[k]), rel_err(r32[k], r64[k])
        b = bound(e32)
        if named and k in named:
            assert named[k] <= CEILING
            b = max(b, named[k])
        print('[persist] %-40s %-12s e = %.2e  e32 = %.2e  (bound %.1e)' % (what, k, e, e32, b))
        if rows is not None:
            rows.append((what, k, e, e32, b))
        if not e <= b:
            errors.append('%s %s: e = %.3e > bound %.3e (e32 = %.3e, K = %g, floor %.0e, ceiling %.0e)'
                          % (what, k, e, b, e32, K, FLOOR, CEILING))
    assert not errors, '\n'.join(errors)


def logit_bound_abs(r64, r32):
    """The logit bound of a case in absolute terms."""
    return bound(rel_err(r32['logits'], r64['logits'])) * float(np.abs(r64['logits']).max())


def check_exact_flags(got, r64, words):
    """live exactly; ended == any(words[1:] == EOS) exactly."""
    assert np.array_equal(np.asarray(got['live']), r64['live']), 'live'
    assert np.array_equal(np.asarray(got['ended']), (np.asarray(words)[1:] == EOS).any(0).astype(np.uint8)), 'ended'


def check_alpha(alpha, mask):
    """Exactly 0 on masked path steps; rows sum to 1 within 1e-6."""
    alpha = np.asarray(alpha, np.float64)
    if mask is not None:
        assert not alpha[:, np.asarray(mask).astype(bool)].any(), 'alpha is not zero on a masked path step'
    assert float(np.abs(alpha.sum(2) - 1.0).max()) <= 1e-6, 'alpha rows do not sum to 1'


def check_argmax_words(words, logits64, bound_abs):
    """Argmax feedback against the float64 logits of the model fed the same words: at every (step, row) the emitted
    word's float64 logit is within 2 x bound of the float64 maximum, and wherever the float64 top-2 margin exceeds
    2 x bound the word IS the float64 arg max."""
    words = np.asarray(words)[1:]
    l = np.asarray(logits64, np.float64)
    assert words.min() >= 0 and words.max() < l.shape[2], 'a word outside [0, vocab)'
    top = np.sort(l, axis=2)[:, :, -2:]
    picked = np.take_along_axis(l, words[:, :, None], 2)[:, :, 0]
    short = top[:, :, 1] - picked
    assert float(short.max()) <= 2 * bound_abs, 'an emitted word lies %.3e below the float64 maximum (2 x bound = %.3e)' % (
        float(short.max()), 2 * bound_abs)
    clear = (top[:, :, 1] - top[:, :, 0]) > 2 * bound_abs
    assert np.array_equal(words[clear], l.argmax(2)[clear]), 'a word is not the float64 arg max at a clear margin'
    return float(clear.mean())


def check_tie_words(words, pair):
    """A tie of the clear maximum: argmax emits the lower index at every step and row."""
    w = np.asarray(words)[1:]
    assert (w == min(pair)).all(), 'a tie between columns %d and %d was not resolved to the lower index: %s' % (
        pair[0], pair[1], np.unique(w))


def check_ctx_beyond_lengths(ctx, lens):
    """pad_packed_sequence: ctx exactly 0 beyond each row's length."""
    ctx = np.asarray(ctx)
    for b, n in enumerate(lens):
        assert not ctx[b, n:].any(), 'ctx of row %d is not zero beyond its length %d' % (b, n)


def check_state_held(hs, cs, lens):
    """hs / cs [T + 1, B, H] carry the state through dead steps exactly."""
    hs, cs = np.asarray(hs), np.asarray(cs)
    for b, n in enumerate(lens):
        assert (hs[n:, b] == hs[n, b]).all() and (cs[n:, b] == cs[n, b]).all(), 'row %d: state not held behind step %d' % (b, n)
