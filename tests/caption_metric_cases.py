"""ROUGE-L and CIDEr-D over BLEU words, restated in plain Python from DESIGN.md section 2: the SPECIFICATION the
package's caption metrics (speaker_evaluation.caption_parts_rows / caption_scores_of, csrc/sf_caption.hip) are held
to, as path_metric_cases.py is for the path metrics.  Sentences are lists of hashable words; nothing here imports the
package, numpy or torch.  The texts come from the g16 fixture (speaker_bleu_cases).

  ROUGE-L   per path, beta = 1.2: lcs_j the longest common subsequence of hypothesis and reference j,
            p = max_j lcs_j / len(hyp), r = max_j lcs_j / len(ref_j), (1 + beta^2) p r / (r + beta^2 p); 0.0 for an empty
            hypothesis or p or r of 0
  CIDEr-D   per path, n = 1..4, sigma = 6: df(g) the number of corpus paths with g in at least one reference,
            idf(g) = log N - log max(1, df(g)); a sentence's vector v_n[g] = tf(g) idf(g) with its norm; against
            reference j val_n = sum over the hypothesis' n-grams of min(vh[g], vr[g]) vr[g], divided by both norms
            when neither is zero, times exp(-(len(hyp) - len(ref_j))^2 / (2 sigma^2)); 10 * mean_n mean_j val_n
  corpus    the paths with exactly instructions_per_path references; the corpus value is the plain mean."""
import math
from collections import Counter

BETA = 1.2
SIGMA = 6.0


def lcs(a, b):
    table = [[0] * (len(b) + 1) for _ in range(len(a) + 1)]
    for i in range(1, len(a) + 1):
        for j in range(1, len(b) + 1):
            if a[i - 1] == b[j - 1]:
                table[i][j] = table[i - 1][j - 1] + 1
            else:
                table[i][j] = max(table[i - 1][j], table[i][j - 1])
    return table[len(a)][len(b)]


def rouge_l(hyp, refs):
    if not hyp:
        return 0.0
    common = [lcs(hyp, ref) for ref in refs]
    p = max(common) / len(hyp)
    r = max(c / len(ref) if ref else 0.0 for c, ref in zip(common, refs))
    if p == 0 or r == 0:
        return 0.0
    return ((1 + BETA ** 2) * p * r) / (r + BETA ** 2 * p)


def ngrams(sentence, n):
    return Counter(tuple(sentence[i:i + n]) for i in range(len(sentence) - n + 1))


def document_frequencies(corpus_refs):
    """Per order the number of corpus paths that hold an n-gram in at least one of their references."""
    df = [Counter() for _ in range(4)]
    for refs in corpus_refs:
        for n in range(1, 5):
            grams = set()
            for ref in refs:
                grams |= set(ngrams(ref, n))
            for g in grams:
                df[n - 1][g] += 1
    return df


def vector(sentence, n, df, n_paths):
    vec = {}
    for g, tf in ngrams(sentence, n).items():
        vec[g] = tf * (math.log(n_paths) - math.log(max(1, df[n - 1].get(g, 0))))
    norm2 = 0.0
    for v in vec.values():
        norm2 += v * v
    return vec, math.sqrt(norm2)


def cider_d(hyp, refs, df, n_paths):
    over_orders = 0.0
    for n in range(1, 5):
        vh, norm_h = vector(hyp, n, df, n_paths)
        over_refs = 0.0
        for ref in refs:
            vr, norm_r = vector(ref, n, df, n_paths)
            val = 0.0
            for g, x in vh.items():
                val += min(x, vr.get(g, 0.0)) * vr.get(g, 0.0)
            if norm_h != 0 and norm_r != 0:
                val /= norm_h * norm_r
            over_refs += val * math.exp(-((len(hyp) - len(ref)) ** 2) / (2 * SIGMA ** 2))
        over_orders += over_refs / len(refs)
    return 10 * (over_orders / 4)


def mean(values):
    values = list(values)
    return math.fsum(values) / len(values) if values else 0.0


def score(corpus_refs, hyps):
    """corpus_refs[i]: the references of scored path i (the whole corpus), hyps[i]: its hypothesis.  Returns the
    per-path (rouge_l, cider_d) lists."""
    df = document_frequencies(corpus_refs)
    return ([rouge_l(h, refs) for refs, h in zip(corpus_refs, hyps)],
            [cider_d(h, refs, df, len(corpus_refs)) for refs, h in zip(corpus_refs, hyps)])


def first_hypotheses(results, instr_ids):
    """path_id -> the words of the first of its instruction ids a walk over `results` meets: what score_results scores."""
    first = {}
    for iid, result in results.items():
        if iid in instr_ids:
            first.setdefault(int(iid.split('_')[0]), result['words'])
    return first
