"""A phoneme duration prior for the Viterbi alignment (`postprocess.duration_prior`): how many frames a phoneme lasts, counted in the
training `.lab` files, as the prior of align.viterbi_align_duration_prior (csrc/align_duration_prior.hip).

Per phoneme the model is P(d), d >= 1 frames: a histogram over d = 1 .. D - 1, and from D on a geometric tail
P(D + i) = P(D) rho^i.  The search adds, for a run of d frames, log P(d) = log_prob[d - 1] for d <= D and log_prob[D - 1] +
(d - D) log_tail beyond.

  estimate     HTK `.lab` files -> DurationPrior (counts, natural-log probabilities)
  flat         a prior that forbids nothing and prefers nothing below D: where `python -m wfl_asr_amd.adapt_durations` starts
  reestimate   expected counts [n, D + 1] (align.duration_prior_expected_counts, summed per phoneme) -> DurationPrior: estimate's
               formula on fractional counts, the M-step of that command
  save / load  the JSON file {"frame_duration", "max_frames", "phonemes": [...], "log_prob": [[D values] | null, ...], "log_tail":
               [...]}; a `null` value is a forbidden duration, a `null` row a phoneme without any sample: no prior
  check        a loaded prior against the label set's output names and the frame clock (ValueError, by name)
  table        DurationPrior -> the float32 [rows][D + 1] table  weight * log P  of the search, -inf kept at every weight
  python -m wfl_asr_amd.durations LAB_DIR... -o phoneme_durations.json [--phonemes phonemes.txt] [--max-frames D] [--smoothing K]
"""
from __future__ import annotations

import json
import math
import os
from typing import List, NamedTuple, Optional

import numpy as np

from .phonotactics import read_lab

MAX_FRAMES = 32            # wfl_align_duration_prior's cap on D


class DurationPrior(NamedTuple):
    frame_duration: float                # seconds per frame the durations were counted on
    max_frames: int                      # D: the longest duration with a histogram entry of its own
    phonemes: List[str]
    log_prob: list                       # per phoneme a float64 [D] array, log P(1) .. log P(D), -inf: forbidden; None: no sample, no prior
    log_tail: np.ndarray                 # [n] float64 log rho, -inf: nothing longer than D (read only where log_prob is a row)
    counts: Optional[list] = None        # per phoneme {frames: count} (estimate); not saved


def frames_of(start_s, end_s, frame_duration) -> int:
    """The frames a segment lasts: max(1, round((end - start) / frame_duration)) (halves go up)."""
    return max(1, int(math.floor((float(end_s) - float(start_s)) / frame_duration + 0.5)))


def _log(p):
    return math.log(p) if p > 0.0 else -math.inf


def _row(c, c_ge, excess, D, K, allowed=None):
    """One phoneme's (log_prob [D], log_tail) from its statistics: c[d - 1] the count of d frames for d < D, c_ge the count of
    d >= D, excess the sum of d - D over those (estimate's docstring has the formula).  allowed: None, or (entries [D] bool, tail
    bool) -- what a prior leaves open: a forbidden entry gets no count and no smoothing and stays -inf, a forbidden tail stays -inf."""
    ok = [True] * D if allowed is None else [bool(x) for x in allowed[0]]
    tail_ok = True if allowed is None else bool(allowed[1])
    c = [c[d] if ok[d] else 0.0 for d in range(D - 1)]
    c_ge = c_ge if ok[D - 1] else 0.0
    n_tot = sum(c) + c_ge
    den = n_tot + K * sum(ok)
    if not den > 0.0:
        return None
    big_m = (c_ge + K) / den if ok[D - 1] else 0.0
    m = (excess + K) / (c_ge + K) if tail_ok and ok[D - 1] and c_ge + K > 0.0 else 0.0
    rho = m / (1.0 + m)
    row = [_log((c[d] + K) / den) if ok[d] else -math.inf for d in range(D - 1)] + [_log(big_m * (1.0 - rho))]
    return np.array(row, np.float64), _log(rho)


def estimate(lab_paths, symbols=None, max_frames=32, smoothing=1.0, frame_duration=0.02) -> DurationPrior:
    """Count the segment durations of HTK `.lab` files.

    symbols         the phonemes to model, in this order.  None: the phonemes the files hold, sorted.  A phoneme of the files that
                    is not among the given symbols is an error
    max_frames      D, 1 .. 32
    smoothing       K, added to every count of a phoneme's histogram (0: a duration never seen is forbidden)
    frame_duration  seconds
    Per phoneme, with c[d] the count of d frames, n_tot their sum and c_ge the count of d >= D:
        P(d) = (c[d] + K) / (n_tot + K D)                          1 <= d < D
        M    = (c_ge + K) / (n_tot + K D)
        m    = (sum over d >= D of (d - D) + K) / (c_ge + K)       (0 / 0 -> 0)
        rho  = m / (1 + m),    P(D) = M (1 - rho),    tail = log rho
    so the probabilities of all d >= 1 sum to 1.  A phoneme without any sample gets no row (None): no prior."""
    D, K = int(max_frames), float(smoothing)
    if not 1 <= D <= MAX_FRAMES:
        raise ValueError(f"max_frames must be 1 .. {MAX_FRAMES}, got {max_frames!r}")
    if not (K >= 0.0 and K < math.inf):
        raise ValueError(f"smoothing must be a finite number >= 0, got {smoothing!r}")
    if not (float(frame_duration) > 0.0 and float(frame_duration) < math.inf):
        raise ValueError(f"frame_duration must be a positive number of seconds, got {frame_duration!r}")
    hist = {}
    for p in lab_paths:
        for start, end, name in read_lab(p):
            h = hist.setdefault(name, {})
            n = frames_of(start, end, float(frame_duration))
            h[n] = h.get(n, 0) + 1
    seen = sorted(hist)
    if symbols is None:
        names = seen
    else:
        names = list(dict.fromkeys(symbols))
        unknown = [s for s in seen if s not in set(names)]
        if unknown:
            raise ValueError(f"the .lab files hold phonemes that are not among the symbols: {', '.join(unknown)}")
    log_prob, log_tail, counts = [], [], []
    for name in names:
        h = hist.get(name, {})
        counts.append(dict(sorted(h.items())))
        n_tot = sum(h.values())
        if n_tot == 0:
            log_prob.append(None)
            log_tail.append(-math.inf)
            continue
        c_ge = sum(c for d, c in h.items() if d >= D)
        excess = sum((d - D) * c for d, c in h.items() if d >= D)
        row, tail = _row([h.get(d, 0) for d in range(1, D)], c_ge, excess, D, K)
        log_prob.append(row)
        log_tail.append(tail)
    return DurationPrior(float(frame_duration), D, list(names), log_prob, np.array(log_tail, np.float64), counts)


def flat(phonemes, max_frames, frame_duration=0.02) -> DurationPrior:
    """Every phoneme the same row: P(d) = 1 / (D + 1) for d < D, P(>= D) = 2 / (D + 1) with rho = 1 / 2.  It sums to 1 and forbids
    nothing."""
    D = int(max_frames)
    if not 1 <= D <= MAX_FRAMES:
        raise ValueError(f"max_frames must be 1 .. {MAX_FRAMES}, got {max_frames!r}")
    names = list(dict.fromkeys(phonemes))
    row = np.full(D, -math.log(D + 1.0), np.float64)          # P(D) = M (1 - rho) = 1 / (D + 1) as well
    return DurationPrior(float(frame_duration), D, names, [row.copy() for _ in names], np.full(len(names), math.log(0.5), np.float64))


def reestimate(counts, phonemes, max_frames, prior=None, prior_count=0.0, smoothing=0.0, frame_duration=0.02) -> DurationPrior:
    """estimate's formula on expected counts: the M-step of `python -m wfl_asr_amd.adapt_durations`.

    counts       float64 [n, D + 1], a row per phoneme in the layout of align.duration_prior_expected_counts' rows: columns 0 .. D - 2
                 the (expected) count of runs of 1 .. D - 1 frames, column D - 1 of runs of D frames or more, column D the sum of
                 d - D over those.  Negative or non-finite counts, or another shape: ValueError
    prior        a DurationPrior over the same phonemes and D, or None.  With it a row receives `prior_count` pseudo-runs spread as
                 the prior's own distribution in the same statistics -- P(d) for d < D, M = P(D) / (1 - rho), excess
                 M rho / (1 - rho) -- and whatever the prior forbids (a null entry, a null tail) stays forbidden, whatever the counts
                 and the smoothing: a forbidden entry takes no count and no smoothing
    smoothing    K of estimate, added to every entry that is not forbidden
    A row whose counts sum to 0 keeps the prior's row; without a prior it is None: no prior.  With integer counts, no prior and the
    same K this is estimate, to the bit."""
    D, K, pc = int(max_frames), float(smoothing), float(prior_count)
    if not 1 <= D <= MAX_FRAMES:
        raise ValueError(f"max_frames must be 1 .. {MAX_FRAMES}, got {max_frames!r}")
    if not (K >= 0.0 and K < math.inf):
        raise ValueError(f"smoothing must be a finite number >= 0, got {smoothing!r}")
    if not (pc >= 0.0 and pc < math.inf):
        raise ValueError(f"prior_count must be a finite number >= 0, got {prior_count!r}")
    if not (float(frame_duration) > 0.0 and float(frame_duration) < math.inf):
        raise ValueError(f"frame_duration must be a positive number of seconds, got {frame_duration!r}")
    names = list(phonemes)
    if len(set(names)) != len(names):
        raise ValueError("phonemes must be distinct")
    cnt = np.asarray(counts, np.float64)
    if cnt.shape != (len(names), D + 1):
        raise ValueError(f"counts must be [{len(names)}, {D + 1}] (phonemes, D + 1), got {list(cnt.shape)}")
    if not np.isfinite(cnt).all() or (cnt < 0).any():
        raise ValueError("counts must be finite and >= 0")
    if prior is not None and (list(prior.phonemes) != names or int(prior.max_frames) != D):
        raise ValueError("the prior must hold the same phonemes in the same order and the same max_frames as the counts")
    if prior is None and pc > 0.0:
        raise ValueError("prior_count needs a prior")
    log_prob, log_tail = [], []
    for i in range(len(names)):
        pr = None if prior is None else prior.log_prob[i]
        c, c_ge, excess = [float(v) for v in cnt[i, :D - 1]], float(cnt[i, D - 1]), float(cnt[i, D])
        out = None
        if sum(c) + c_ge > 0.0:
            allowed = None
            if pr is not None:
                lt = float(prior.log_tail[i])
                allowed = (np.isfinite(pr), np.isfinite(lt))
                if pc > 0.0:
                    rho = math.exp(lt)
                    if not rho < 1.0:
                        raise ValueError(f"{names[i]}: the prior's tail is rho = 1, no distribution to spread prior_count by")
                    big_m = math.exp(pr[D - 1]) / (1.0 - rho)
                    c = [v + pc * math.exp(pr[d]) for d, v in enumerate(c)]
                    c_ge, excess = c_ge + pc * big_m, excess + pc * big_m * rho / (1.0 - rho)
            out = _row(c, c_ge, excess, D, K, allowed)
        if out is None:                            # no count (or none on an entry the prior leaves open): the prior's row
            log_prob.append(None if pr is None else np.array(pr, np.float64))
            log_tail.append(-math.inf if pr is None else float(prior.log_tail[i]))
        else:
            log_prob.append(out[0])
            log_tail.append(out[1])
    return DurationPrior(float(frame_duration), D, names, log_prob, np.array(log_tail, np.float64))


def save(prior: DurationPrior, path):
    def num(v):
        return float(v) if np.isfinite(v) else None
    rows = [None if r is None else [num(v) for v in r] for r in prior.log_prob]
    tails = [None if r is None else num(t) for r, t in zip(prior.log_prob, prior.log_tail)]
    d = os.path.dirname(os.path.abspath(path))
    os.makedirs(d, exist_ok=True)
    with open(path, "w", encoding="utf-8") as f:
        f.write('{"frame_duration": ' + json.dumps(float(prior.frame_duration)) + ', "max_frames": ' + json.dumps(int(prior.max_frames)))
        f.write(',\n "phonemes": ' + json.dumps(list(prior.phonemes), ensure_ascii=False) + ',\n "log_prob": [\n')   # one row per line
        f.write(",\n".join("  " + json.dumps(r) for r in rows) + "\n ],\n")
        f.write(' "log_tail": ' + json.dumps(tails) + "}\n")


def load(path) -> DurationPrior:
    with open(path, "r", encoding="utf-8") as f:
        d = json.load(f)
    try:
        fd, D, names, rows, tails = float(d["frame_duration"]), int(d["max_frames"]), list(d["phonemes"]), d["log_prob"], d["log_tail"]
    except (KeyError, TypeError, ValueError):
        raise ValueError(f'{path}: not a phoneme duration file ({{"frame_duration", "max_frames", "phonemes": [...], '
                         '"log_prob": [[...]], "log_tail": [...]})')
    n = len(names)
    if not 1 <= D <= MAX_FRAMES:
        raise ValueError(f"{path}: max_frames must be 1 .. {MAX_FRAMES}")
    if not (fd > 0.0 and fd < math.inf):
        raise ValueError(f"{path}: frame_duration must be a positive number of seconds")
    if len(set(names)) != n:
        raise ValueError(f"{path}: phonemes must be distinct")
    if not isinstance(rows, list) or not isinstance(tails, list) or len(rows) != n or len(tails) != n \
            or any(r is not None and (not isinstance(r, list) or len(r) != D) for r in rows):
        raise ValueError(f"{path}: log_prob must hold {n} rows of {D} values (or null), log_tail {n} values")
    lp = [None if r is None else np.array([-np.inf if v is None else float(v) for v in r], np.float64) for r in rows]
    lt = np.array([-np.inf if v is None else float(v) for v in tails], np.float64)
    if any(r is not None and (np.isnan(r).any() or np.isposinf(r).any()) for r in lp) or np.isnan(lt).any() or (lt > 0).any():
        raise ValueError(f"{path}: log_prob holds a NaN or +inf, or log_tail a NaN or a value above 0 (a forbidden duration is null)")
    return DurationPrior(fd, D, names, lp, lt)


def check(prior: DurationPrior, output_names, frame_duration, path="the duration prior"):
    """A prior is usable with a label set and a frame clock: its frame_duration is the clock's, and every phoneme it holds is an
    output name of the label set (ValueError, naming the phonemes, otherwise)."""
    if abs(float(prior.frame_duration) - float(frame_duration)) > 1e-9:
        raise ValueError(f"{path}: counted on frames of {prior.frame_duration:g} s, the model's frames last {float(frame_duration):g} s; "
                         "estimate it again with that frame duration")
    known = set(output_names)
    unknown = [p for p in prior.phonemes if p not in known]
    if unknown:
        raise ValueError(f"{path}: holds phonemes that are no output name of the label set: {', '.join(unknown)}")


def table(prior: DurationPrior, weight=1.0) -> np.ndarray:
    """The float32 [rows][D + 1] table of align.viterbi_align_duration_prior: row i is  weight * (log P(1) .. log P(D), log rho)  of
    phoneme i.  A forbidden duration stays -inf at every weight, 0 included; a phoneme without samples keeps a row of zeros that
    align.duration_rows never points at."""
    w = float(weight)
    if not (w >= 0.0 and w < math.inf):
        raise ValueError(f"duration_prior_weight must be a finite number >= 0, got {weight!r}")
    D = int(prior.max_frames)
    out = np.zeros((len(prior.phonemes), D + 1), np.float64)
    for i, r in enumerate(prior.log_prob):
        if r is None:
            continue
        v = np.concatenate([np.asarray(r, np.float64), [float(prior.log_tail[i])]])
        out[i] = np.where(np.isneginf(v), -np.inf, w * np.where(np.isneginf(v), 0.0, v))
    return out.astype(np.float32)


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m wfl_asr_amd.durations",
                                 description="Estimate phoneme duration histograms from HTK .lab files for postprocess.duration_prior")
    ap.add_argument("lab_dirs", nargs="+", metavar="LAB_DIR", help="folders searched for *.lab (recursively), or .lab files")
    ap.add_argument("-o", "--output", required=True, help="the JSON file to write")
    ap.add_argument("--phonemes", help="the model's phonemes.txt (one BIO label per line): emit every phoneme of the label set, in its "
                                       "order; one without any sample gets no prior")
    ap.add_argument("--max-frames", type=int, default=32, help="D: durations up to D frames get a histogram entry, longer ones a "
                                                               "geometric tail (default 32, the most the search holds)")
    ap.add_argument("--smoothing", type=float, default=1.0, help="added to every count (default 1; 0 forbids what was never seen)")
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
        prior = estimate(paths, symbols, a.max_frames, a.smoothing)
    except ValueError as err:
        ap.error(str(err))
    save(prior, a.output)
    empty = [p for p, r in zip(prior.phonemes, prior.log_prob) if r is None]
    if empty:
        print(f"no sample, no prior: {', '.join(empty)}")
    n_seg = sum(sum(c.values()) for c in prior.counts)
    print(f"{len(paths)} .lab files, {n_seg} segments, {len(prior.phonemes) - len(empty)} phonemes with a prior -> {a.output}")


if __name__ == "__main__":
    main()
