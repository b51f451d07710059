"""Scoring of speaker results (tasks/R2R/eval_speaker.py:11-122): corpus BLEU of one generated instruction per path
against the path's reference instructions, and the mean of the model's own scores.

The reference writes hypotheses and references to temporary files, pipes them through a perl script (bleu.py:15-72)
and parses the one line it prints.  Corpus BLEU is a function of TEN INTEGERS per corpus -- clipped n-gram matches and
n-gram totals for n = 1..4, the hypothesis length, the closest reference length -- so here

  * `split_sentence`, `bleu_words`   the tokeniser's splitting rule (utils.py:71-90) and the re-split the script applies
                                     to the blank-joined lines (a token that holds a blank counts as two BLEU words)
  * `bleu_count_rows`                the ten integers per path in plain Python: the SPECIFICATION of sf_bleu_counts
                                     (csrc/sf_bleu.hip), which counts them on the device
  * `bleu_from_counts`               the only floating point of the module: the script's formula, in its order, in
                                     float64, and bleu.py's parse of the printed line ('%.2f' / '%.3f') -- host and device
                                     counting both end here, so they agree bit for bit whenever their integers agree
  * `multi_bleu`, `single_bleu`      bleu.py's functions: no subprocess, no files
  * `SpeakerEvaluation`              eval_speaker.py's class: `score_results`, `score_file` with the reference's contract,
                                     and `score_speaker`: agent.test() + score_results as one device sweep with one host
                                     sync, the words counted where the decode left them.
  * `caption_parts_rows`             (no reference counterpart) the parts of ROUGE-L and CIDEr-D per path in plain Python:
                                     the SPECIFICATION of sf_caption_scores (csrc/sf_caption.hip); `caption_corpus` and
                                     `caption_static_rows` are what they need of the references alone
  * `caption_scores_of`              the one place the two scores are formed, for host and device counting alike;
                                     `SpeakerEvaluation(..., caption_metrics=True)` is the switch

Nothing here imports torch before a device is asked for, and nothing imports the reference.
"""
import ctypes as C
import json
import math
import re
import string
from collections import Counter

import numpy as np

DATA_JSON = 'tasks/R2R/data/R2R_%s.json'                                 # utils.py:54-59
ROW = ('correct1', 'correct2', 'correct3', 'correct4', 'total1', 'total2', 'total3', 'total4', 'hyp_len', 'ref_len')

_SENTENCE_SPLIT = re.compile(r'(\W+)')                                   # utils.py:71
_BLANKS = re.compile('[ \t\n\r\f\v]+')                                   # what the script's `split` splits on (bytes)


def split_sentence(sentence):
    """utils.Tokenizer.split_sentence (utils.py:80-90): lower-cased words and punctuation; a run of punctuation is
    broken into its characters unless it is made of full stops only."""
    toks = []
    for word in [s.strip().lower() for s in _SENTENCE_SPLIT.split(sentence.strip()) if len(s.strip()) > 0]:
        if all(c in string.punctuation for c in word) and not all(c in '.' for c in word):
            toks += list(word)
        else:
            toks.append(word)
    return toks


def bleu_words(tokens):
    """The words the script sees: bleu.py joins the tokens of a sentence with blanks (bleu.py:51, 56) and the script
    splits the line on white space again -- a token that holds a blank ('. .') is two BLEU words, an empty one none."""
    return [w for w in _BLANKS.split(' '.join(tokens)) if w]


def bleu_count_rows(refs, hyps):
    """refs[i]: the reference sentences of path i, hyps[i]: its hypothesis; sentences are lists of BLEU words (any
    hashable: strings, ids).  Returns int32 [N, 10]: per path correct_1..4, total_1..4, hyp_len, closest_ref_len --
    the script's per-sentence additions to CORRECT[n], TOTAL[n], length_translation and length_reference."""
    rows = np.zeros((len(hyps), 10), np.int32)
    for i, (sentences, hyp) in enumerate(zip(refs, hyps)):
        H = len(hyp)
        closest_diff, closest_length = 9999, 9999
        ref_ngram = {}                                       # n-gram -> its largest count in a single reference
        for ref in sentences:
            length = len(ref)
            diff = abs(H - length)
            if diff < closest_diff:
                closest_diff, closest_length = diff, length
            elif diff == closest_diff and length < closest_length:
                closest_length = length                      # (the shorter of two equally close references)
            for n in range(1, 5):
                for gram, k in Counter(tuple(ref[s:s + n]) for s in range(length - n + 1)).items():
                    if ref_ngram.get(gram, 0) < k:
                        ref_ngram[gram] = k
        for n in range(1, 5):
            t_ngram = Counter(tuple(hyp[s:s + n]) for s in range(H - n + 1))
            rows[i, 3 + n] = sum(t_ngram.values())
            rows[i, n - 1] = sum(min(k, ref_ngram.get(gram, 0)) for gram, k in t_ngram.items())
        rows[i, 8], rows[i, 9] = H, closest_length
    return rows


def _my_log(x):
    return math.log(x) if x else -9999999999


def bleu_from_counts(sums):
    """sums: the ten integers of a corpus (ROW order).  Returns (bleu, unpenalized_bleu, record): the pair is what
    bleu.call_bleu parses from the line the script prints -- bleu = float('%.2f' % (100 * BLEU)), the brevity penalty
    rounded to three decimals, unpenalized = the quotient of those two ROUNDED numbers; (0, 0) where the script prints
    nothing (a reference length above 0 with a hypothesis length of 0: it dies on a division by zero) -- and `record`
    holds the unrounded numbers: bleu_exact (0..1), precisions, brevity_penalty, hyp_len, ref_len."""
    s = [int(x) for x in sums]
    correct, total, hyp_len, ref_len = s[0:4], s[4:8], s[8], s[9]
    precisions = [correct[n] / total[n] if total[n] else 0.0 for n in range(4)]
    record = dict(bleu_exact=0.0, precisions=precisions, brevity_penalty=0.0, hyp_len=hyp_len, ref_len=ref_len)
    if ref_len == 0:                                         # "BLEU = 0, 0/0/0/0 (BP=0, ..."
        return 0.0, 0, record
    if hyp_len == 0:                                         # 1 - ref_len / 0: no line, "BLEU score not found"
        return 0, 0, record
    brevity_penalty = math.exp(1 - ref_len / hyp_len) if hyp_len < ref_len else 1
    exact = brevity_penalty * math.exp((_my_log(precisions[0]) + _my_log(precisions[1]) + _my_log(precisions[2]) +
                                        _my_log(precisions[3])) / 4)
    record.update(bleu_exact=exact, brevity_penalty=float(brevity_penalty))
    bleu = float('%.2f' % (100 * exact))
    bp = float('%.3f' % brevity_penalty)
    return bleu, (bleu / bp if bp != 0 else 0), record


def multi_bleu(multiple_references, hypotheses):
    """bleu.multi_bleu (bleu.py:41-68): sentences are token lists; returns (bleu, unpenalized_bleu)."""
    num_refs = len(multiple_references[0])
    assert (all(len(refs) == num_refs for refs in multiple_references))
    if num_refs == 0:                                        # no reference file: the script dies, nothing is printed
        return 0, 0
    rows = bleu_count_rows([[bleu_words(r) for r in refs] for refs in multiple_references],
                           [bleu_words(h) for h in hypotheses])
    return bleu_from_counts(rows.sum(0, dtype=np.int64))[:2]


def single_bleu(references, hypotheses):
    return multi_bleu([[ref] for ref in references], hypotheses)


# --------------------------------------------------------------------------------- caption metrics: ROUGE-L and CIDEr-D
CAPTION_BETA = 1.2                                                       # ROUGE-L's weight of recall
CAPTION_SIGMA = 6.0                                                      # CIDEr-D's length penalty
PARTS = ('hyp_len', 'lcs', 'dot', 'hnorm2')


def _ngram_counts(sentence, n):
    """n-gram -> its count, in the order of first occurrence."""
    return Counter(tuple(sentence[s:s + n]) for s in range(len(sentence) - n + 1))


def _lcs(a, b):
    """The length of the longest common subsequence: the full dynamic program, row by row."""
    prev = [0] * (len(b) + 1)
    for x in a:
        cur = [0]
        for j, y in enumerate(b):
            cur.append(max(cur[j], prev[j] + 1 if x == y else prev[j + 1]))
        prev = cur
    return prev[-1]


def caption_corpus(refs):
    """refs[i]: the reference sentences of scored path i -- the corpus CIDEr-D's document frequencies are counted over.
    Returns n_paths (N), log_n and idf: per order n = 1..4 a dictionary n-gram -> log N - log max(1, df), df the number
    of paths that hold the n-gram in at least one reference.  An n-gram outside the dictionary has df 0: idf log_n."""
    N = len(refs)
    log_n = math.log(N) if N else 0.0
    idf = []
    for n in range(1, 5):
        df = Counter()
        for sentences in refs:
            df.update({gram for ref in sentences for gram in _ngram_counts(ref, n)})
        idf.append({gram: log_n - math.log(max(1, k)) for gram, k in df.items()})
    return dict(n_paths=N, log_n=log_n, idf=idf)


def caption_static_rows(refs, corpus):
    """What the two metrics need of the references alone, per path: ref_len [R] and ref_norm [R][4], the norm of every
    reference's tf-idf vector per order.  Static per evaluator; never on the device."""
    rows = []
    for sentences in refs:
        norms = []
        for ref in sentences:
            norms.append([])
            for n in range(1, 5):
                idf, acc = corpus['idf'][n - 1], 0.0
                for gram, k in _ngram_counts(ref, n).items():
                    v = k * idf.get(gram, corpus['log_n'])
                    acc += v * v
                norms[-1].append(math.sqrt(acc))
        rows.append(dict(ref_len=[len(ref) for ref in sentences], ref_norm=norms))
    return rows


def caption_parts_rows(refs, hyps, corpus=None):
    """refs[i]: the reference sentences of path i, hyps[i]: its hypothesis (lists of BLEU words: any hashable); corpus:
    `caption_corpus` of the evaluator's scored paths (None: of `refs` themselves).  Returns per path the PARTS the two
    metrics are functions of -- the SPECIFICATION of sf_caption_scores (csrc/sf_caption.hip):
      hyp_len        the number of words of the hypothesis
      lcs [R]        the LCS length of the hypothesis and reference j
      hnorm2 [4]     per order the sum over the hypothesis' distinct n-grams g of (tf_h(g) idf(g))^2
      dot [R][4]     per reference and order the sum over the same g of min(tf_h idf, tf_j idf) * (tf_j idf)
    The sums run over the n-grams in the order of their first occurrence in the hypothesis; every term is >= 0."""
    corpus = caption_corpus(refs) if corpus is None else corpus
    rows = []
    for sentences, hyp in zip(refs, hyps):
        hnorm2, dot = [0.0] * 4, [[0.0] * 4 for _ in sentences]
        for n in range(1, 5):
            idf = corpus['idf'][n - 1]
            tf_refs = [_ngram_counts(ref, n) for ref in sentences]
            for gram, k in _ngram_counts(hyp, n).items():
                w = idf.get(gram, corpus['log_n'])
                vh = k * w
                hnorm2[n - 1] += vh * vh
                for j, tf in enumerate(tf_refs):
                    vr = tf.get(gram, 0) * w
                    dot[j][n - 1] += min(vh, vr) * vr
        rows.append(dict(hyp_len=len(hyp), lcs=[_lcs(hyp, ref) for ref in sentences], dot=dot, hnorm2=hnorm2))
    return rows


def caption_scores_of(parts, static):
    """THE place where the two scores of a path are formed: parts (a row of caption_parts_rows, or what
    sf_caption_scores wrote for the path) and static (the path's row of caption_static_rows) -> (rouge_l, cider_d).
    Host and device counting both end here, so ROUGE-L -- a function of integers -- agrees bit for bit, and CIDEr-D
    to the rounding of the sums in `dot` and `hnorm2`."""
    H, lcs, ref_len = int(parts['hyp_len']), [int(x) for x in parts['lcs']], static['ref_len']
    rouge_l = 0.0
    if H > 0 and lcs:
        p = max(lcs) / H
        r = max(k / L if L else 0.0 for k, L in zip(lcs, ref_len))
        if p > 0 and r > 0:
            rouge_l = ((1 + CAPTION_BETA ** 2) * p * r) / (r + CAPTION_BETA ** 2 * p)
    total = 0.0
    for n in range(4):
        hnorm = math.sqrt(float(parts['hnorm2'][n]))
        over_refs = 0.0
        for j, L in enumerate(ref_len):
            val = float(parts['dot'][j][n])
            rnorm = static['ref_norm'][j][n]
            if hnorm != 0 and rnorm != 0:
                val /= hnorm * rnorm
            over_refs += val * math.exp(-((H - L) ** 2) / (2 * CAPTION_SIGMA ** 2))
        total += over_refs / len(ref_len) if ref_len else 0.0
    return rouge_l, 10 * (total / 4)


def caption_mean(values):
    """The corpus value: the plain mean over the scored paths (the exactly rounded sum over their number)."""
    values = list(values)
    return math.fsum(values) / len(values) if values else 0.0


# ----------------------------------------------------------------------------------------------- counting on the device
def _cuda_device(device):
    """The torch device to count on, or None: `device` as given, else the current GPU when there is one."""
    import torch
    if device is None:
        return torch.device('cuda', torch.cuda.current_device()) if torch.cuda.is_available() else None
    device = torch.device(device)
    return device if device.type == 'cuda' else None


def bleu_limits():
    """(dictionary size, words per hypothesis, words per reference, references per path) sf_bleu_counts takes."""
    from . import _lib
    lib = _lib.lib
    return lib.sf_bleu_max_dict(), lib.sf_bleu_max_hyp(), lib.sf_bleu_max_ref(), lib.sf_bleu_max_refs()


def _packed(sentences):
    """(ids int32, offsets int32 [n + 1]) of id lists; ids holds at least one element (a device pointer is never NULL)."""
    off = np.zeros(len(sentences) + 1, np.int32)
    np.cumsum([len(s) for s in sentences], out=off[1:])
    ids = np.fromiter((w for s in sentences for w in s), np.int32, int(off[-1]))
    return (ids if len(ids) else np.zeros(1, np.int32)), off


def _fitting(refs, hyps, ids):
    """The paths inside the kernels' limits (`fit`) and the others (`rest`), with the references and hypotheses of the
    former as ids: `ids` (word -> id) is extended by every new word, in path order."""
    max_dict, max_hyp, max_ref, max_refs = bleu_limits()
    R = len(refs[0])
    fit, rest, ref_ids, hyp_ids = [], [], [], []
    for i, (sentences, hyp) in enumerate(zip(refs, hyps)):
        ok = (len(sentences) == R and 1 <= R <= max_refs and len(hyp) <= max_hyp
              and all(len(s) <= max_ref for s in sentences))
        if ok:
            known = len(ids)
            mine = [[ids.setdefault(w, len(ids)) for w in s] for s in list(sentences) + [hyp]]
            if len(ids) > max_dict:                          # this path's new words no longer fit the key packing
                for w in [w for w, k in ids.items() if k >= known]:
                    del ids[w]
                ok = False
        if ok:
            fit.append(i)
            ref_ids += mine[:-1]
            hyp_ids.append(mine[-1])
        else:
            rest.append(i)
    return fit, rest, ref_ids, hyp_ids, R, ids


def count_rows(refs, hyps, device=None):
    """`bleu_count_rows(refs, hyps)` with the paths inside sf_bleu_counts' limits counted on `device` (None: the
    current GPU when there is one, else everything on the host) and the others on the host and merged.  Returns
    (rows int32 [N, 10], indices of the paths counted on the host)."""
    N = len(hyps)
    dev = _cuda_device(device) if N else None
    if dev is None:
        return bleu_count_rows(refs, hyps), list(range(N))
    fit, rest, ref_ids, hyp_ids, R, ids = _fitting(refs, hyps, {})
    rows = np.zeros((N, 10), np.int32)
    if fit:
        got = _device_rows(ref_ids, hyp_ids, R, len(ids), dev)
        if got is None:                                      # (SF_ERR_UNSUPPORTED after all: the limits moved)
            fit, rest = [], list(range(N))
        else:
            rows[fit] = got
    if rest:
        rows[rest] = bleu_count_rows([refs[i] for i in rest], [hyps[i] for i in rest])
    return rows, rest


def _device_rows(ref_ids, hyp_ids, R, n_dict, dev):
    """One sf_bleu_counts over packed hypotheses (path i in slot i); None where the library refuses the shapes."""
    import torch
    from . import _lib
    from .runtime import stream
    N = len(hyp_ids)
    r_ids, r_off = _packed(ref_ids)
    h_ids, h_off = _packed(hyp_ids)
    with torch.cuda.device(dev):
        up = [torch.from_numpy(a).to(dev) for a in (h_ids, h_off, r_ids, r_off, np.arange(N, dtype=np.int32))]
        rows = torch.zeros(N, 10, dtype=torch.int32, device=dev)
        sums = torch.zeros(10, dtype=torch.int64, device=dev)
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        b = _lib.BleuBatch(n_hyps=N, n_slots=N, n_refs=R, n_dict=max(1, n_dict),
                           max_hyp=int(np.diff(h_off).max()), max_ref=int(np.diff(r_off).max()),
                           hyp_ids=up[0].data_ptr(), hyp_off=up[1].data_ptr(), ref_ids=up[2].data_ptr(),
                           ref_off=up[3].data_ptr(), slot=up[4].data_ptr(), rows=rows.data_ptr(), sums=sums.data_ptr())
        rc = _lib.lib.sf_bleu_counts(C.byref(b), C.c_void_p(err.data_ptr()), stream())
        if rc == _lib.SF_ERR_UNSUPPORTED:
            return None
        _lib.check(rc, 'sf_bleu_counts')
        out = torch.cat((rows.reshape(-1).to(torch.int64), sums, err.to(torch.int64))).cpu().numpy()   # (the one sync)
    if out[-1]:
        raise RuntimeError('sf_bleu_counts: an id outside its dictionary, or a length above the limits')
    got = out[:N * 10].reshape(N, 10).astype(np.int32)
    if (got.sum(0, dtype=np.int64) != out[N * 10:N * 10 + 10]).any():
        raise RuntimeError('sf_bleu_counts: the sums are not the sums of the rows')
    return got


def caption_key_tables(corpus, ids):
    """The idf dictionaries of a corpus as sf_caption_scores takes them: per order the unique keys (the packing of the
    n-gram's ids, first word lowest), sorted, the four tables one behind the other, and the idf of every key."""
    keys, idf, n_keys = [], [], []
    for n in range(4):
        table = sorted((sum(ids[w] << (16 * k) for k, w in enumerate(gram)), v) for gram, v in corpus['idf'][n].items())
        keys += [k for k, _ in table]
        idf += [v for _, v in table]
        n_keys.append(len(table))
    return dict(keys=np.array(keys or [0], np.uint64), idf=np.array(idf or [0.0], np.float64), n_keys=n_keys,
                log_n=corpus['log_n'], on_device={})


def _device_parts(ref_ids, hyp_ids, R, n_dict, tables, dev):
    """One sf_caption_scores over packed hypotheses (path i in slot i): the rows of caption_parts_rows; None where the
    library refuses the shapes.  The key tables go to a device once."""
    import torch
    from . import _lib
    from .runtime import stream
    N = len(hyp_ids)
    r_ids, r_off = _packed(ref_ids)
    h_ids, h_off = _packed(hyp_ids)
    with torch.cuda.device(dev):
        if str(dev) not in tables['on_device']:
            tables['on_device'][str(dev)] = (torch.from_numpy(tables['keys'].view(np.int64)).to(dev),
                                             torch.from_numpy(tables['idf']).to(dev))
        keys, idf = tables['on_device'][str(dev)]
        up = [torch.from_numpy(a).to(dev) for a in (h_ids, h_off, r_ids, r_off, np.arange(N, dtype=np.int32))]
        ints = torch.zeros(N * (1 + R) + 1, dtype=torch.int32, device=dev)          # hyp_len, lcs, err
        reals = torch.zeros(N * (R * 4 + 4), dtype=torch.float64, device=dev)       # dot, hnorm2
        k = tables['n_keys']
        b = _lib.CaptionBatch(n_hyps=N, n_slots=N, n_refs=R, n_dict=max(1, n_dict),
                              max_hyp=int(np.diff(h_off).max()), max_ref=int(np.diff(r_off).max()),
                              hyp_ids=up[0].data_ptr(), hyp_off=up[1].data_ptr(), ref_ids=up[2].data_ptr(),
                              ref_off=up[3].data_ptr(), slot=up[4].data_ptr(), n_keys1=k[0], n_keys2=k[1], n_keys3=k[2],
                              n_keys4=k[3], keys=keys.data_ptr(), idf=idf.data_ptr(), idf_miss=tables['log_n'],
                              hyp_len=ints.data_ptr(), lcs=ints[N:].data_ptr(), dot=reals.data_ptr(),
                              hnorm2=reals[N * R * 4:].data_ptr())
        rc = _lib.lib.sf_caption_scores(C.byref(b), C.c_void_p(ints[N * (1 + R):].data_ptr()), stream())
        if rc == _lib.SF_ERR_UNSUPPORTED:
            return None
        _lib.check(rc, 'sf_caption_scores')
        out = torch.cat((ints.to(torch.float64), reals)).cpu().numpy()              # (the one sync; int32 is exact)
    ints, reals = out[:len(ints)].astype(np.int64), out[len(ints):]
    if ints[-1]:
        raise RuntimeError('sf_caption_scores: an id outside its dictionary, or a length above the limits')
    return _parts_of(ints[:N], ints[N:N * (1 + R)].reshape(N, R), reals[:N * R * 4].reshape(N, R, 4),
                     reals[N * R * 4:].reshape(N, 4))


def _parts_of(hyp_len, lcs, dot, hnorm2):
    """The kernel's four output arrays as the rows caption_parts_rows returns."""
    return [dict(hyp_len=int(hyp_len[i]), lcs=[int(x) for x in lcs[i]], dot=[[float(x) for x in d] for d in dot[i]],
                 hnorm2=[float(x) for x in hnorm2[i]]) for i in range(len(hyp_len))]


# ----------------------------------------------------------------------------------------------- eval_speaker.py:11-122
def _paths_of(items):
    """The first item of each path_id, in order.  An env holds one item per instruction, with the instruction's text
    as a string (env.py:679-684): the path's list is put together again in instruction order."""
    first, texts = {}, {}
    for it in items:
        pid = it['path_id']
        ins = it.get('instructions')
        if isinstance(ins, str):
            j = int(str(it['instr_id']).split('_')[-1]) if 'instr_id' in it else len(texts.get(pid, {}))
            texts.setdefault(pid, {})[j] = ins
        if pid not in first:
            first[pid] = it
    out = []
    for pid, it in first.items():
        it = dict(it)
        if pid in texts:
            it['instructions'] = [texts[pid][j] for j in sorted(texts[pid])]
        out.append(it)
    return out


class SpeakerEvaluation(object):
    """eval_speaker.py:11-122.  Results: {instr_id: {'words': [...], optionally 'score'}}.

    SpeakerEvaluation(splits, instructions_per_path=None)   reads tasks/R2R/data/R2R_<split>.json relative to the
                                                            working directory (the reference's form)
    SpeakerEvaluation(env=env)                              the items of an env (one per instruction: the first item of
                                                            each path_id is kept, the path's instructions regrouped)
    SpeakerEvaluation(items=...)                            items with 'path_id', 'scan', 'instructions'
    device: where score_results counts (None: the current GPU when there is one, else the host; 'cpu': the host).
    caption_metrics: also score ROUGE-L and CIDEr-D over the scored paths: the summary gains
    'rouge_l' and 'cider_d', `captions` holds the per-path parts and scores.  Off, nothing is computed or launched."""

    def __init__(self, splits=None, instructions_per_path=None, env=None, items=None, device=None,
                 caption_metrics=False):
        if env is not None:
            items = _paths_of(env.data) if items is None else items
            splits = list(getattr(env, 'splits', [])) if splits is None else splits
        elif items is None:
            items = []
            for split in splits:
                with open(DATA_JSON % split) as f:
                    items += json.load(f)
        else:
            items = _paths_of(items)
        self.splits = splits if splits is not None else []
        self.gt = {}
        self.instr_ids = []
        self.scans = []
        if instructions_per_path is None:
            instructions_per_path = 3
        self.instructions_per_path = instructions_per_path
        for item in items:
            item = dict(item)
            item['instructions'] = item['instructions'][:instructions_per_path]
            self.gt[item['path_id']] = item
            self.scans.append(item['scan'])
            self.instr_ids += ['%d_%d' % (item['path_id'], i) for i in range(len(item['instructions']))]
        self.scans = set(self.scans)
        self.instr_ids = set(self.instr_ids)
        self._device = device
        self._refs = {}                                      # path_id -> the BLEU words of its references
        self.counts = None
        self.fallbacks = 0
        self.host_syncs = self.last_host_syncs = self.sweeps = 0
        self._sweep_tables = {}
        self.caption_metrics = bool(caption_metrics)
        self.captions = None
        self._caption = None                                 # what the caption metrics need of the references alone

    def _references(self, base_id):
        refs = self._refs.get(base_id)
        if refs is None:
            refs = self._refs[base_id] = [bleu_words(split_sentence(ref)) for ref in self.gt[base_id]['instructions']]
        return refs

    def _set_counts(self, path_ids, rows, on_host):
        rows = np.asarray(rows, np.int32).reshape(len(path_ids), 10)
        self.counts = dict(rows={pid: rows[i] for i, pid in enumerate(path_ids)}, sums=rows.sum(0, dtype=np.int64),
                           on_host=[path_ids[i] for i in on_host])
        return self.counts['sums']

    def score_results(self, results, verbose=False):
        """results: instr_id -> dictionary with (at least) 'words'.  Returns (summary, instruction_replaced_gt) as the
        reference does; `self.counts` then holds the ten integers per scored path ('rows', keyed by path_id), their
        'sums' and the paths counted on the host ('on_host': all of them without a GPU, else those above the kernel's
        limits)."""
        instr_ids = set(self.instr_ids)
        instr_count = 0
        results_by_base_id = {}
        mismatches = []
        for instr_id, result in results.items():
            if instr_id in instr_ids:
                instr_ids.remove(instr_id)
                base_id = int(instr_id.split('_')[0])
                if base_id in results_by_base_id:
                    old_predicted = results_by_base_id[base_id]['words']
                    new_predicted = result['words']
                    if old_predicted != new_predicted:
                        mismatches.append((old_predicted, new_predicted))
                else:
                    results_by_base_id[base_id] = result
        if mismatches:
            print("mismatching outputs for sentences:")
            for old_pred, new_pred in mismatches:
                print(old_pred)
                print(new_pred)
                print()
        assert len(instr_ids) == 0, 'Missing %d of %d instruction ids from %s' % (
            len(instr_ids), len(self.instr_ids), ",".join(self.splits))
        all_refs, all_hyps, scored = [], [], []
        model_scores = []
        instruction_replaced_gt = []
        skip_count = 0
        skipped_refs = set()
        for base_id, result in sorted(results_by_base_id.items()):
            instr_count += 1
            gt = self.gt[base_id]
            tokenized_hyp = result['words']
            replaced_gt = gt.copy()
            replaced_gt['instructions'] = [' '.join(tokenized_hyp)]
            instruction_replaced_gt.append(replaced_gt)
            if 'score' in result:
                model_scores.append(result['score'])
            if len(gt['instructions']) != self.instructions_per_path:
                skip_count += 1
                skipped_refs.add(base_id)
                continue
            all_refs.append(self._references(base_id))
            all_hyps.append(bleu_words(tokenized_hyp))
            scored.append(base_id)
            if verbose and instr_count % 100 == 0:
                for i, ref in enumerate(split_sentence(ref) for ref in gt['instructions']):
                    print("ref {}:\t{}".format(i, ' '.join(ref)))
                print("pred  :\t{}".format(' '.join(tokenized_hyp)))
                print()
        if skip_count != 0:
            print("skipped {} instructions without {} refs: {}".format(
                skip_count, self.instructions_per_path, ' '.join(str(i) for i in skipped_refs)))
        model_score = np.mean(model_scores)
        self.skipped = sorted(skipped_refs)
        rows, on_host = count_rows(all_refs, all_hyps, self._device)
        if self.caption_metrics:
            self._set_captions(scored, *self._caption_parts(scored, all_refs, all_hyps))
        return self._summary(model_score, self._set_counts(scored, rows, on_host)), instruction_replaced_gt

    def _summary(self, model_score, sums):
        bleu, unpenalized_bleu, self.bleu_record = bleu_from_counts(sums)
        summary = {'model_score': model_score, 'bleu': bleu, 'unpenalized_bleu': unpenalized_bleu}
        if self.caption_metrics:
            summary['rouge_l'] = caption_mean(self.captions['rouge_l'].values())
            summary['cider_d'] = caption_mean(self.captions['cider_d'].values())
        return summary

    # ---- ROUGE-L and CIDEr-D (caption_metrics=True)
    def _caption_static(self):
        """Built once per evaluator: the scored paths (exactly instructions_per_path references; sorted), the corpus
        their references make (document frequencies -> idf), every path's static row, and the dictionary of the
        reference words in the order _sweep_table numbers them -- the ids the key tables are packed from."""
        if self._caption is None:
            scored = [pid for pid in sorted(self.gt) if len(self.gt[pid]['instructions']) == self.instructions_per_path]
            refs = [self._references(pid) for pid in scored]
            corpus = caption_corpus(refs)
            ids = {}
            for sentences in refs:
                for ref in sentences:
                    for w in ref:
                        ids.setdefault(w, len(ids))
            self._caption = dict(scored=scored, corpus=corpus, ids=ids, tables=None,
                                 static=dict(zip(scored, caption_static_rows(refs, corpus))))
        return self._caption

    def _caption_tables(self):
        """The key tables of the corpus, or None where they do not fit: a reference dictionary above the kernel's."""
        st = self._caption_static()
        if len(st['ids']) > bleu_limits()[0]:
            return None
        if st['tables'] is None:
            st['tables'] = caption_key_tables(st['corpus'], st['ids'])
        return st['tables']

    def _caption_parts(self, scored, refs, hyps):
        """`caption_parts_rows` over the evaluator's corpus, with the paths inside the kernel's limits on the device
        and the others on the host and merged, as count_rows does for BLEU.  Returns (parts, indices on the host)."""
        st = self._caption_static()
        N = len(hyps)
        dev = _cuda_device(self._device) if N else None
        tables = self._caption_tables() if dev is not None else None
        if tables is None:
            return caption_parts_rows(refs, hyps, st['corpus']), list(range(N))
        fit, rest, ref_ids, hyp_ids, R, ids = _fitting(refs, hyps, dict(st['ids']))
        parts = [None] * N
        if fit:
            got = _device_parts(ref_ids, hyp_ids, R, len(ids), tables, dev)
            if got is None:                                  # (SF_ERR_UNSUPPORTED after all: the limits moved)
                fit, rest = [], list(range(N))
            for i, row in zip(fit, got or []):
                parts[i] = row
        for i, row in zip(rest, caption_parts_rows([refs[i] for i in rest], [hyps[i] for i in rest], st['corpus'])):
            parts[i] = row
        return parts, rest

    def _set_captions(self, path_ids, parts, on_host):
        static = self._caption_static()['static']
        scores = [caption_scores_of(row, static[pid]) for pid, row in zip(path_ids, parts)]
        self.captions = dict(parts=dict(zip(path_ids, parts)), rouge_l={pid: s[0] for pid, s in zip(path_ids, scores)},
                             cider_d={pid: s[1] for pid, s in zip(path_ids, scores)},
                             on_host=[path_ids[i] for i in on_host])

    def score_file(self, output_file, verbose=False):
        with open(output_file) as f:
            return self.score_results(json.load(f), verbose=verbose)

    # ---- agent.test() + score_results as one device sweep
    @staticmethod
    def _vocabulary(agent):
        """The word of every vocabulary id as test() would decode it (Tokenizer.decode_sentence), or None."""
        tok = getattr(agent.env, 'tokenizer', None)
        if tok is None:
            return None
        from .follower import EOS
        n = agent.decoder.vocab_size
        vocab = getattr(tok, 'vocab', None)
        if vocab is not None and len(vocab) >= n:
            return [vocab[v] for v in range(n)]
        return [None if v == EOS else tok.decode_sentence([v], break_on_eos=True, join=False)[0] for v in range(n)]

    def _sweep_table(self, agent, dev):
        """The device side of a sweep that does not depend on the results: the dictionary (every BLEU word of the
        references and of the vocabulary, by string), the references of the scored paths as packed ids, one slot per
        scored path in sorted path_id order, the vocabulary-id -> dictionary-ids table (train_vocab.txt holds the token
        '. .': two BLEU words).  None where the kernel's limits do not hold it, or a vocabulary word is more than two
        BLEU words."""
        import torch
        vocab = self._vocabulary(agent)
        if vocab is None:
            return None
        key = (str(dev), id(agent.env.tokenizer), len(vocab), agent.instruction_len)
        t = self._sweep_tables.get(key)
        if t is not None:
            return t if t else None
        max_dict, max_hyp, max_ref, max_refs = bleu_limits()
        R = self.instructions_per_path
        scored = [pid for pid in sorted(self.gt) if len(self.gt[pid]['instructions']) == R]
        ids, ok = {}, 1 <= R <= max_refs and len(scored) > 0
        tables = None
        if self.caption_metrics:                             # the key tables are packed from these ids: start from them
            tables = self._caption_tables()
            ids, ok = dict(self._caption_static()['ids']), ok and tables is not None
        refs = []
        for pid in scored if ok else []:
            for ref in self._references(pid):
                ok = ok and len(ref) <= max_ref
                refs.append([ids.setdefault(w, len(ids)) for w in ref])
        remap = np.full((len(vocab), 2), -1, np.int32)       # a vocabulary word is no, one or two BLEU words
        for v, word in enumerate(vocab if ok else []):
            if word is None:                                 # (EOS: never part of a hypothesis)
                continue
            parts = bleu_words([word])
            if len(parts) > 2:
                ok = False
                break
            remap[v, :len(parts)] = [ids.setdefault(w, len(ids)) for w in parts]
        longest = agent.instruction_len * (2 if (remap[:, 1] >= 0).any() else 1)
        if not ok or len(ids) > max_dict or longest > max_hyp:
            self._sweep_tables[key] = False
            return None
        r_ids, r_off = _packed(refs)
        with torch.cuda.device(dev):
            t = dict(n_dict=len(ids), n_slots=len(scored), slot_of={pid: i for i, pid in enumerate(scored)},
                     scored=scored, max_ref=int(np.diff(r_off).max()), max_hyp=longest, n_vocab=len(vocab), vocab=vocab,
                     ref_ids=torch.from_numpy(r_ids).to(dev), ref_off=torch.from_numpy(r_off).to(dev),
                     remap=torch.from_numpy(remap).to(dev),
                     rows=torch.zeros(len(scored), 10, dtype=torch.int32, device=dev),
                     out=torch.zeros(12, dtype=torch.int64, device=dev),             # sums [10], err, (unused)
                     rows_h=torch.zeros(len(scored), 10, dtype=torch.int32).pin_memory(),
                     out_h=torch.zeros(12, dtype=torch.int64).pin_memory())
            if tables is not None:                           # hyp_len, lcs | dot, hnorm2 of every slot
                if str(dev) not in tables['on_device']:
                    tables['on_device'][str(dev)] = (torch.from_numpy(tables['keys'].view(np.int64)).to(dev),
                                                     torch.from_numpy(tables['idf']).to(dev))
                n = len(scored)
                t.update(tables=tables, cap_i=torch.zeros(n * (1 + R), dtype=torch.int32, device=dev),
                         cap_f=torch.zeros(n * (R * 4 + 4), dtype=torch.float64, device=dev),
                         cap_i_h=torch.zeros(n * (1 + R), dtype=torch.int32).pin_memory(),
                         cap_f_h=torch.zeros(n * (R * 4 + 4), dtype=torch.float64).pin_memory())
        self._sweep_tables = {key: t}
        return t

    def _sweepable(self, agent, use_dropout, feedback):
        """The feature store to sweep on, or None: the conditions of Seq2SeqSpeaker._test_as_a_sweep other than the
        number of minibatches."""
        store = agent._env_store() if hasattr(agent, '_env_store') else None
        env = agent.env
        if (use_dropout or feedback != 'argmax' or store is None or not getattr(agent, 'index_gold_routes', False)
                or getattr(env, 'host_table', 1) is not None or not hasattr(env, 'graphs') or not hasattr(env, 'data')
                or store.device.type != 'cuda' or not len(env.data)):
            return None
        return store

    def _by_test(self, agent, use_dropout, feedback):
        self.fallbacks += 1
        agent.test(use_dropout=use_dropout, feedback=feedback)
        return self.score_results(agent.results)

    def score_speaker(self, agent, use_dropout=False, feedback='argmax', keep_results=False):
        """What `agent.test(use_dropout, feedback)` followed by `score_results(agent.results)` returns, as ONE sweep on
        the device: the environment is drawn exactly as Seq2SeqSpeaker._test_as_a_sweep draws it (reset_epoch, then
        sweeps.epoch_minibatches -- `env.ix` and `random` end where test() leaves them), every minibatch is decoded through
        speaker.SpeakerSweep whatever `sweep_test_after` says, sf_bleu_counts is issued behind each minibatch's replay
        on the same stream and reads the words where the decode left them (a path's slot goes to the FIRST of its
        instruction ids the walk meets; ids already issued, ids outside `instr_ids` and skipped paths write nothing),
        and the host waits ONCE, after the last minibatch (`last_host_syncs`; the capture of a route length nobody has
        captured yet synchronises on its own).  model_score is np.mean over the same float scores in sorted path_id
        order as score_results takes it.  `agent.losses` is set as test() sets it; `agent.results` stays empty unless
        keep_results.  The second return value, instruction_replaced_gt, is built from the kept results: it is None
        with keep_results=False.  The words of a path's other instruction ids never leave the device, so the sweep
        does not print score_results' "mismatching outputs" report (a path decoded in two minibatches of different
        route lengths may come out in different words; the first one met is the path's hypothesis either way).

        An agent _test_as_a_sweep would not take (dropout, feedback other than argmax, a dense environment, no
        tokenizer), a dictionary or lengths above sf_bleu_counts' limits, or a raised fault word mean agent.test() +
        score_results instead (`fallbacks`): a faulting sweep is never scored, and the environment's item order and
        `random` are put back first, so that test() walks what the sweep walked."""
        store = self._sweepable(agent, use_dropout, feedback)
        table = self._sweep_table(agent, store.device) if store is not None else None
        if table is None:
            return self._by_test(agent, use_dropout, feedback)
        import torch
        from . import _lib, speaker as spk
        from .follower import EOS
        from .runtime import stream, clear_faults, download_faults, take_fault
        from .sweeps import epoch_minibatches, snapshot, restore
        env, dev = agent.env, store.device
        agent.feedback = feedback
        for m in (agent.encoder, agent.decoder):
            m.eval()
        agent.beam_size = 1
        walk0 = snapshot(env)                                # (a faulting sweep is undone: test() then walks from here)
        env.reset_epoch()
        agent.losses, agent.results = [], {}
        B, S = env.batch_size, agent.instruction_len
        drawn = []
        first_of = {}                                        # path_id -> (minibatch, column) of its first result
        for k, items, fresh in epoch_minibatches(env):       # (speaker.py:404-413 over the items themselves)
            for b, it in enumerate(items):
                if fresh[b] and it['instr_id'] in self.instr_ids:
                    first_of.setdefault(int(it['instr_id'].split('_')[0]), (k, b))
            drawn.append(items)
        agent._test_minibatches = agent.__dict__.get('_test_minibatches', 0) + len(drawn)
        missing = self.instr_ids - {it['instr_id'] for items in drawn for it in items}
        assert len(missing) == 0, 'Missing %d of %d instruction ids from %s' % (
            len(missing), len(self.instr_ids), ",".join(self.splits))
        K = len(drawn)
        slots = np.full((K, B), -1, np.int32)
        for pid, (k, b) in first_of.items():
            slots[k, b] = table['slot_of'].get(pid, -1)
        key = (id(store), B, S, agent.wide_sample)
        cached = agent.__dict__.get('_test_sweep')
        if cached is None or cached[0] != key:
            cached = agent._test_sweep = (key, spk.SpeakerSweep(agent.encoder, agent.decoder, store, B, S,
                                                                feedback='argmax', Lmax=S, with_scores=True,
                                                                wide_sample=agent.wide_sample), store)
        sweep = cached[1]
        sweep.ensure_slots(-(-K // len(sweep.streams)))      # (no wait for a staging buffer in the middle of the sweep)
        with torch.cuda.device(dev):
            slots_d = torch.from_numpy(slots).pin_memory().to(dev, non_blocking=True)
            table['rows'].zero_()
            table['out'].zero_()
            if self.caption_metrics:
                table['cap_i'].zero_()
                table['cap_f'].zero_()
            clear_faults(dev)
            ptr_of = lambda x: x.data_ptr()                  # noqa: E731

            def count(k, st):
                """Behind minibatch k's replay, on its stream: the words are read where the decode left them."""
                b = _lib.BleuBatch(n_hyps=B, n_slots=table['n_slots'], n_refs=self.instructions_per_path,
                                   n_dict=table['n_dict'], max_hyp=table['max_hyp'], max_ref=table['max_ref'], S=S,
                                   word_bytes=8,
                                   eos=EOS, n_vocab=table['n_vocab'], words=ptr_of(st.words[1:]),
                                   remap=ptr_of(table['remap']), ref_ids=ptr_of(table['ref_ids']),
                                   ref_off=ptr_of(table['ref_off']), slot=ptr_of(slots_d[k]), rows=ptr_of(table['rows']),
                                   sums=ptr_of(table['out']))
                _lib.call('sf_bleu_counts', C.byref(b), C.c_void_p(ptr_of(table['out'][10:11])), stream())
                if self.caption_metrics:                     # next to it: the same words, slots and fault word
                    n, R, nk = table['n_slots'], self.instructions_per_path, table['tables']['n_keys']
                    keys, idf = table['tables']['on_device'][str(dev)]
                    c = _lib.CaptionBatch(n_hyps=B, n_slots=n, n_refs=R, n_dict=table['n_dict'],
                                          max_hyp=table['max_hyp'], max_ref=table['max_ref'], S=S, word_bytes=8, eos=EOS,
                                          n_vocab=table['n_vocab'], words=b.words, remap=b.remap, ref_ids=b.ref_ids,
                                          ref_off=b.ref_off, slot=b.slot, n_keys1=nk[0], n_keys2=nk[1], n_keys3=nk[2],
                                          n_keys4=nk[3], keys=ptr_of(keys), idf=ptr_of(idf),
                                          idf_miss=table['tables']['log_n'], hyp_len=ptr_of(table['cap_i']),
                                          lcs=ptr_of(table['cap_i'][n:]), dot=ptr_of(table['cap_f']),
                                          hnorm2=ptr_of(table['cap_f'][n * R * 4:]))
                    _lib.call('sf_caption_scores', C.byref(c), C.c_void_p(ptr_of(table['out'][10:11])), stream())
            handle = sweep.issue([agent._routes_of(items, store)[0] for items in drawn], after=count,
                                 clear_faults=False)
            tail = sweep.streams[(K - 1) % len(sweep.streams)]
            for s in sweep.streams:
                tail.wait_stream(s)
            with torch.cuda.stream(tail):
                table['rows_h'].copy_(table['rows'], non_blocking=True)
                table['out_h'].copy_(table['out'], non_blocking=True)
                if self.caption_metrics:
                    table['cap_i_h'].copy_(table['cap_i'], non_blocking=True)
                    table['cap_f_h'].copy_(table['cap_f'], non_blocking=True)
                fpin = download_faults(dev)
            tail.synchronize()                               # the one host sync of the sweep
        self.sweeps += 1
        out = table['out_h'].numpy()
        if any(fpin.tolist()) or int(out[10]):
            take_fault(dev)                                  # (read and cleared: test() starts clean)
            self.last_host_syncs = 2
            self.host_syncs += 2
            restore(env, walk0)
            return self._by_test(agent, use_dropout, feedback)
        self.last_host_syncs = 1
        self.host_syncs += 1
        words, scores, cnt = handle['out'].numpy(), handle['scores'].numpy(), handle['cnt'].numpy()
        score_of = {}
        for k, items in enumerate(drawn):
            both = np.concatenate((words[k].astype(np.float32), scores[k]), axis=0)
            outputs, loss = agent._score_outputs([it['instr_id'] for it in items], both, S, None, cnt[k], dev)
            agent.loss = loss
            agent.losses.append(float(loss))
            for b, result in enumerate(outputs):
                score_of[(k, b)] = result['score']
                if keep_results and result['instr_id'] not in agent.results:
                    agent.results[result['instr_id']] = result
        model_score = np.mean([score_of[first_of[pid]] for pid in sorted(first_of)])
        scored = [pid for pid in table['scored'] if pid in first_of]
        rows = table['rows_h'].numpy()[[table['slot_of'][pid] for pid in scored]].copy()
        sums = self._set_counts(scored, rows, [])
        if (sums != out[:10]).any():
            raise RuntimeError('sf_bleu_counts: the sums are not the sums of the rows')
        if self.caption_metrics:
            n, R = table['n_slots'], self.instructions_per_path
            ints, reals = table['cap_i_h'].numpy(), table['cap_f_h'].numpy()
            parts = _parts_of(ints[:n], ints[n:].reshape(n, R), reals[:n * R * 4].reshape(n, R, 4),
                              reals[n * R * 4:].reshape(n, 4))
            self._set_captions(scored, [parts[table['slot_of'][pid]] for pid in scored], [])
        self.skipped = sorted(pid for pid in first_of if pid not in table['slot_of'])
        if self.skipped:
            print("skipped {} instructions without {} refs: {}".format(
                len(self.skipped), self.instructions_per_path, ' '.join(str(i) for i in set(self.skipped))))
        replaced = None
        if keep_results:
            replaced = []
            for pid in sorted(first_of):
                k, b = first_of[pid]
                gt = self.gt[pid].copy()
                gt['instructions'] = [' '.join(agent.results[drawn[k][b]['instr_id']]['words'])]
                replaced.append(gt)
        return self._summary(model_score, sums), replaced
