"""A phone bigram for the BIO-grammar decode (`postprocess.phoneme_bigram`): which phoneme follows which, counted in the training
`.lab` files, as the prior of decode.bio_viterbi_bigram (csrc/decode_bigram.hip).

Symbols are `O` (silence between segments: no phoneme) and the phonemes.  The model is P(next symbol | previous symbol) over the
successions the search pays for: every opened phoneme run, and every `O` run after a phoneme.  `O` after `O` is no succession.

  estimate          HTK `.lab` files -> Bigram (counts, natural-log conditional probabilities)
  reestimate        expected succession counts (decode.bigram_expected_counts, summed over unlabelled audio) -> Bigram: the M-step
                    of adapt_bigram.py, with an optional prior bigram
  save / load       the JSON file {"symbols": ["O", ...], "log_prob": [[...]]}, `null` = a forbidden succession
  transition_table  Bigram + the label set's class table -> the float32 table  weight * log_prob - switch_penalty  of the search
  python -m wfl_asr_amd.phonotactics LAB_DIR... -o phoneme_bigram.json [--phonemes phonemes.txt] [--smoothing K] [--min-gap S]
"""
from __future__ import annotations

import json
import os
from typing import List, NamedTuple, Optional

import numpy as np

HTK_TIME_FACTOR = 1e7      # .lab times are in 100 ns units
O = "O"


class Bigram(NamedTuple):
    symbols: List[str]                   # "O" first, then the phonemes
    log_prob: np.ndarray                 # [n, n] float64, rows the previous symbol; -inf: forbidden; [O][O] is -inf (never read)
    counts: Optional[np.ndarray] = None  # [n, n] int64 (estimate), float64 (reestimate); not saved


def read_lab(path):
    """-> [(start_s, end_s, name)] of an HTK label file (blank and malformed lines are passed over)."""
    segs = []
    with open(path, "r", encoding="utf-8") as f:
        for line in f:
            parts = line.split()
            if len(parts) >= 3:
                try:
                    segs.append((float(parts[0]) / HTK_TIME_FACTOR, float(parts[1]) / HTK_TIME_FACTOR, parts[2]))
                except ValueError:
                    continue
    return segs


def successions(segments, min_gap=0.02):
    """The (previous symbol, next symbol) pairs of one file's segments.  The file starts after `O`; a gap of at least `min_gap` seconds
    between two segments, or before the first one, is `O`; equal neighbours are p -> p."""
    out, prev, prev_end = [], O, 0.0
    for start, end, name in segments:
        if start - prev_end >= min_gap and prev != O:
            out.append((prev, O))
            prev = O
        out.append((prev, name))
        prev, prev_end = name, end
    return out


def estimate(lab_paths, symbols=None, smoothing=1.0, min_gap=0.02) -> Bigram:
    """Count the successions of HTK `.lab` files.

    symbols    the phonemes to model, in this order (an `O` among them is ignored; `O` is always symbol 0).  None: the phonemes the
               files hold, sorted.  A phoneme of the files that is not among the given symbols is an error.
    smoothing  added to every count of a row, over all next symbols except `O` -> `O` (0: a succession never seen is forbidden)
    min_gap    seconds; a shorter gap between two segments is no `O`
    -> Bigram with natural-log conditional probabilities log P(next | previous)."""
    if not float(smoothing) >= 0.0:
        raise ValueError(f"smoothing must be >= 0, got {smoothing!r}")
    pairs = []
    for p in lab_paths:
        pairs += successions(read_lab(p), min_gap)
    seen = sorted({b for _, b in pairs if b != O})
    if symbols is None:
        names = seen
    else:
        names = [s for s in dict.fromkeys(symbols) if s != O]
        unknown = [s for s in seen if s not in set(names)]
        if unknown:
            raise ValueError(f"the .lab files hold phonemes that are not among the symbols: {', '.join(unknown)}")
    syms = [O] + list(names)
    idx = {s: i for i, s in enumerate(syms)}
    n = len(syms)
    counts = np.zeros((n, n), np.int64)
    for a, b in pairs:
        counts[idx[a], idx[b]] += 1
    c = counts.astype(np.float64) + float(smoothing)
    c[0, 0] = 0.0
    tot = c.sum(axis=1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        lp = np.where(c > 0, np.log(c / tot), -np.inf)
    return Bigram(syms, lp, counts)


def reestimate(counts, symbols, prior: Optional[Bigram] = None, prior_count=0.0, smoothing=0.0) -> Bigram:
    """Expected succession counts -> Bigram, as `estimate` turns its integer counts into one.

    counts       float64 [n, n] in `symbols`' order ("O" first), rows the previous symbol, entries >= 0
    prior        a Bigram over the same symbols in the same order: a succession it forbids stays forbidden, whatever the counts and
                 the smoothing; prior_count pseudo-successions per row are spread as its probabilities
    smoothing    added to every allowed count of a row
    Row by row  c = counts + prior_count * exp(prior.log_prob) + smoothing,  normalised over the row; `O` -> `O` is excluded.  A row
    whose total is 0 keeps the prior's row; without a prior it is uniform over its allowed successions.  ValueError, naming the
    phoneme, when a [p][O] that the prior allows (every one, without a prior) would come out forbidden: the search needs a way into
    `O` from every phoneme."""
    syms = list(symbols)
    n = len(syms)
    if n == 0 or syms[0] != O or len(set(syms)) != n:
        raise ValueError("symbols must be distinct and begin with 'O'")
    c = np.array(counts, np.float64)
    if c.shape != (n, n):
        raise ValueError(f"counts must be a [{n}, {n}] table, got {list(c.shape)}")
    if not np.isfinite(c).all() or (c < 0).any():
        raise ValueError("counts must be finite and >= 0")
    if not float(prior_count) >= 0.0 or not float(smoothing) >= 0.0:
        raise ValueError("prior_count and smoothing must be >= 0")
    allowed = np.ones((n, n), bool)
    pp = np.zeros((n, n))
    if prior is not None:
        if list(prior.symbols) != syms:
            raise ValueError("the prior bigram must hold the same symbols in the same order")
        lp0 = np.asarray(prior.log_prob, np.float64)
        allowed = np.isfinite(lp0)
        pp = np.where(allowed, np.exp(np.where(allowed, lp0, 0.0)), 0.0)
    allowed[0, 0] = False
    pp[0, 0] = 0.0
    c = np.where(allowed, c + (float(prior_count) * pp if float(prior_count) > 0.0 else 0.0) + float(smoothing), 0.0)
    tot = c.sum(axis=1, keepdims=True)
    empty = tot[:, 0] == 0
    if empty.any():                                  # nothing seen from this symbol: the prior's row, else uniform
        fill = pp if prior is not None else allowed.astype(np.float64)
        c[empty] = fill[empty]
        tot = c.sum(axis=1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        lp = np.where(c > 0, np.log(c / tot), -np.inf)
    shut = [syms[p] for p in range(1, n) if allowed[p, 0] and not np.isfinite(lp[p, 0])]
    if shut:
        raise ValueError(f"no way into 'O' is left from: {', '.join(shut)} (use smoothing > 0 or a prior_count > 0)")
    return Bigram(syms, lp, np.array(counts, np.float64))


def save(bigram: Bigram, path):
    lp = np.asarray(bigram.log_prob, np.float64)
    rows = [[float(v) if np.isfinite(v) else None for v in row] for row in lp]
    d = os.path.dirname(os.path.abspath(path))
    os.makedirs(d, exist_ok=True)
    with open(path, "w", encoding="utf-8") as f:
        f.write('{"symbols": ' + json.dumps(list(bigram.symbols), ensure_ascii=False) + ',\n "log_prob": [\n')     # one row per line
        f.write(",\n".join("  " + json.dumps(r) for r in rows) + "\n ]}\n")


def load(path) -> Bigram:
    with open(path, "r", encoding="utf-8") as f:
        d = json.load(f)
    try:
        syms, rows = list(d["symbols"]), d["log_prob"]
    except (KeyError, TypeError):
        raise ValueError(f'{path}: not a phoneme bigram file ({{"symbols": [...], "log_prob": [[...]]}})')
    n = len(syms)
    if n == 0 or syms[0] != O or len(set(syms)) != n:
        raise ValueError(f"{path}: symbols must be distinct and begin with 'O'")
    if len(rows) != n or any(len(r) != n for r in rows):
        raise ValueError(f"{path}: log_prob must be a {n} x {n} table")
    lp = np.array([[-np.inf if v is None else float(v) for v in r] for r in rows], np.float64).reshape(n, n)
    if np.isnan(lp).any() or np.isposinf(lp).any():
        raise ValueError(f"{path}: log_prob holds a NaN or +inf (a forbidden succession is null)")
    return Bigram(syms, lp)


def transition_table(bigram: Bigram, class_table, label_list, switch_penalty=0.0, weight=1.0) -> np.ndarray:
    """The float32 table of decode.bio_viterbi_bigram: W[previous][opened] = weight * log_prob - switch_penalty, symbol 0 being O and
    symbol 1 + p the phoneme of class_table.pairs[p] (decode.class_table(label_list)).  A forbidden succession stays -inf; with weight
    0 the table is -switch_penalty everywhere (the plain search).  ValueError, naming the symbols, when a phoneme of the label set is
    missing from the bigram or the bigram holds a symbol the label set lacks."""
    if not float(weight) >= 0.0:
        raise ValueError(f"bigram_weight must be >= 0, got {weight!r}")
    if not float(switch_penalty) >= 0.0:
        raise ValueError(f"switch_penalty must be >= 0, got {switch_penalty!r}")
    _, pairs = class_table
    names = [label_list[int(b)][2:] for b, _ in np.asarray(pairs).reshape(-1, 2)]
    idx = {s: i for i, s in enumerate(bigram.symbols)}
    missing = [s for s in names if s not in idx]
    if missing:
        raise ValueError(f"the phoneme bigram lacks phonemes of the label set: {', '.join(missing)}")
    unknown = [s for s in bigram.symbols if s != O and s not in set(names)]
    if unknown:
        raise ValueError(f"the phoneme bigram holds symbols the label set lacks: {', '.join(unknown)}")
    order = [idx[O]] + [idx[s] for s in names]
    lp = np.asarray(bigram.log_prob, np.float64)[np.ix_(order, order)]
    if float(weight) == 0.0:
        w = np.zeros_like(lp)
    else:
        w = np.where(np.isneginf(lp), -np.inf, float(weight) * np.where(np.isneginf(lp), 0.0, lp))
    w[0, 0] = 0.0                                   # O after O is never read
    return (w - float(switch_penalty)).astype(np.float32)


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m wfl_asr_amd.phonotactics",
                                 description="Estimate a phone bigram from HTK .lab files for postprocess.phoneme_bigram")
    ap.add_argument("lab_dirs", nargs="+", metavar="LAB_DIR", help="folders searched for *.lab (recursively), or .lab files")
    ap.add_argument("-o", "--output", required=True, help="the JSON file to write")
    ap.add_argument("--phonemes", help="the model's phonemes.txt (one BIO label per line): emit every phoneme of the label set, in its "
                                       "order, so the file always loads with that model")
    ap.add_argument("--smoothing", type=float, default=1.0, help="added to every count (default 1; 0 forbids what was never seen)")
    ap.add_argument("--min-gap", type=float, default=0.02, help="seconds between two segments from which the gap is O (default 0.02)")
    a = ap.parse_args(argv)
    paths = []
    for d in a.lab_dirs:
        if os.path.isdir(d):
            for dp, _, fs in sorted(os.walk(d)):
                paths += [os.path.join(dp, f) for f in sorted(fs) if f.lower().endswith(".lab")]
        else:
            paths.append(d)
    if not paths:
        ap.error("no .lab file found")
    symbols = None
    if a.phonemes:
        from .decode import class_table
        with open(a.phonemes, "r", encoding="utf-8") as f:
            labels = [ln.strip() for ln in f if ln.strip()]
        symbols = [labels[int(b)][2:] for b, _ in class_table(labels).pairs]
    try:
        bg = estimate(paths, symbols, a.smoothing, a.min_gap)
    except ValueError as err:
        ap.error(str(err))
    save(bg, a.output)
    print(f"{len(paths)} .lab files, {int(bg.counts.sum())} successions, {len(bg.symbols) - 1} phonemes -> {a.output}")


if __name__ == "__main__":
    main()
