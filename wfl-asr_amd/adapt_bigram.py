"""Adapt the phone bigram of the BIO-grammar decode (`postprocess.phoneme_bigram`) to audio WITHOUT labels: Baum-Welch re-estimation
over the grammar the bigram search runs on.

phonotactics.estimate counts successions in the training `.lab` files.  Who has only a checkpoint and recordings of their own -- a new
singer, another language mix -- has no such files.  One EM round here forwards the audio, lets the GPU sum, over every legal path
weighted by its probability, how often symbol q is opened directly after symbol s (Labeler.expected_successions, decode.
bigram_expected_counts, csrc/decode_bigram_counts.hip), and turns those expected counts into a bigram exactly as estimate turns its
integer counts into one (phonotactics.reestimate).  The result is a phoneme_bigram.json like any other.

  adapt   the loop: start table -> [transition_table, expected_successions, reestimate] x iterations -> (Bigram, one record per round)
  python -m wfl_asr_amd.adapt_bigram AUDIO... -ckpt best_model.pt -c config.yaml -o adapted.json
         [--init phoneme_bigram.json] [--iterations K=3] [--prior-count M=0] [--smoothing S=0.1]
         [--bigram-weight W] [--switch-penalty L] [--lang-id ID] [--confidence-threshold T]

Every round forwards the audio again; the logits are not kept between rounds.
"""
from __future__ import annotations

import os
from typing import List, NamedTuple

import numpy as np

from . import phonotactics as PH
from .decode import MAX_BIGRAM_SYMBOLS, class_table

AUDIO_EXT = (".wav",)


class Round(NamedTuple):
    files: int              # files that were counted
    frames: int
    successions: float      # the expected number of opened runs, all files
    nats_per_frame: float   # (sum logZ - sum lse) / frames: the log mass the grammar and the table keep, per frame
    skipped: List[str]


def symbols_of(labels) -> List[str]:
    """"O" and the phonemes of the label set in the order of decode.class_table: the symbols of the search's table."""
    return [PH.O] + [labels[int(b)][2:] for b, _ in class_table(labels).pairs]


def uniform_bigram(symbols) -> PH.Bigram:
    """Every succession equally likely (`O` -> `O` excluded, as everywhere)."""
    n = len(symbols)
    allowed = np.ones((n, n), bool)
    allowed[0, 0] = False
    with np.errstate(divide="ignore"):
        lp = np.where(allowed, -np.log(np.maximum(allowed.sum(axis=1, keepdims=True), 1)), -np.inf)
    return PH.Bigram(list(symbols), lp)


def start_bigram(labels, init_path=None) -> PH.Bigram:
    """The start table in the symbols' order of the label set, checked before any forward: a label set over the search's cap, an
    `init` file that does not fit the label set (phonotactics.transition_table's rule) or that decode.check_transitions refuses is a
    ValueError."""
    from .decode import check_transitions
    syms = symbols_of(labels)
    if len(syms) > MAX_BIGRAM_SYMBOLS:
        raise ValueError(f"the label set has {len(syms) - 1} phonemes; the bigram search takes at most {MAX_BIGRAM_SYMBOLS - 1}")
    if init_path is None:
        return uniform_bigram(syms)
    bg = PH.load(init_path)
    ct = class_table(labels)
    try:
        check_transitions(PH.transition_table(bg, ct, labels), len(ct.pairs))
    except ValueError as err:
        raise ValueError(f"{init_path}: {err}")
    idx = [bg.symbols.index(s) for s in syms]
    return PH.Bigram(syms, np.asarray(bg.log_prob, np.float64)[np.ix_(idx, idx)])


def find_audio(paths) -> List[str]:
    """The audio files among `paths`: a file as it is, a folder's *.wav (sorted, not recursive)."""
    out = []
    for p in paths:
        if os.path.isdir(p):
            out += [os.path.join(p, f) for f in sorted(os.listdir(p)) if f.lower().endswith(AUDIO_EXT)]
        elif os.path.isfile(p):
            out.append(p)
    return out


def adapt(labeler, audio_paths, start: PH.Bigram, iterations=3, prior_count=0.0, smoothing=0.1, bigram_weight=1.0, switch_penalty=0.0,
          lang_id=None, confidence_threshold=0.0, use_prior=False, verbose=True, report=None):
    """The EM loop -> (Bigram, [Round]).  start: start_bigram's result; it is also the prior of every re-estimation when use_prior
    (an --init file was given).  report(round number, Round) is called after every round."""
    ct = class_table(labeler.labels)
    bg, rounds = start, []
    for k in range(int(iterations)):
        trans = PH.transition_table(bg, ct, labeler.labels, switch_penalty, bigram_weight)
        counts, logz, lse, frames, skipped = labeler.expected_successions(audio_paths, trans, lang_id, confidence_threshold, verbose)
        rec = Round(len(audio_paths) - len(skipped), frames, float(counts.sum()), (logz - lse) / max(frames, 1), list(skipped))
        rounds.append(rec)
        if report is not None:
            report(k + 1, rec)
        bg = PH.reestimate(counts, start.symbols, start if use_prior else None, prior_count, smoothing)
    return bg, rounds


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(
        prog="python -m wfl_asr_amd.adapt_bigram",
        description="Re-estimate the phone bigram of --decode viterbi on audio without labels (Baum-Welch over the decode's grammar, on "
                    "the GPU). Prints one line per round: files, frames, expected successions and (sum logZ - sum lse) / frames in nats "
                    "per frame. With --bigram-weight 1, --switch-penalty 0, --smoothing 0 and --prior-count 0 that figure cannot "
                    "decrease from round to round (the EM bound); with any other setting it is informative only.")
    ap.add_argument("audio", nargs="+", metavar="AUDIO", help="audio files, or folders whose *.wav files are taken")
    ap.add_argument("-ckpt", "--checkpoint", required=True, help="the model checkpoint")
    ap.add_argument("-c", "--config", required=True, help="the model's config.yaml")
    ap.add_argument("-o", "--output", required=True, help="the phoneme_bigram.json to write")
    ap.add_argument("--init", help="a phoneme_bigram.json to start from; it is also the prior of every round, and what it forbids stays "
                                   "forbidden (default: every succession equally likely)")
    ap.add_argument("--iterations", type=int, default=3, help="EM rounds; every round forwards the audio again (default 3)")
    ap.add_argument("--prior-count", type=float, default=0.0, help="pseudo-successions per row taken from --init (default 0)")
    ap.add_argument("--smoothing", type=float, default=0.1, help="added to every allowed expected count (default 0.1)")
    ap.add_argument("--bigram-weight", type=float, default=None, help="default: config postprocess.bigram_weight, else 1")
    ap.add_argument("--switch-penalty", type=float, default=None, help="default: config postprocess.switch_penalty, else 0")
    ap.add_argument("--lang-id", type=int, default=None, help="language id (default: the average over all languages)")
    ap.add_argument("--confidence-threshold", type=float, default=None, help="default: config postprocess.confidence_threshold, else 0")
    ap.add_argument("--device", default="cuda")
    a = ap.parse_args(argv)
    if a.iterations < 1:
        ap.error("--iterations must be >= 1")
    if not a.prior_count >= 0.0 or not a.smoothing >= 0.0:
        ap.error("--prior-count and --smoothing must be >= 0")
    if a.prior_count > 0.0 and not a.init:
        ap.error("--prior-count needs --init")
    from . import postprocess as pp
    from .infer import load_config
    if not os.path.isfile(a.config):
        ap.error(f"config file not found: {a.config}")
    cfg = load_config(a.config)
    post = cfg.get("postprocess") or {}
    weight = post.get("bigram_weight") if a.bigram_weight is None else a.bigram_weight
    weight = 1.0 if weight is None else float(weight)
    penalty = float(post.get("switch_penalty", 0.0) if a.switch_penalty is None else a.switch_penalty)
    threshold = float(post.get("confidence_threshold", 0.0) if a.confidence_threshold is None else a.confidence_threshold)
    if not weight >= 0.0 or not penalty >= 0.0 or not threshold >= 0.0:
        ap.error("--bigram-weight, --switch-penalty and --confidence-threshold must be >= 0")
    labels = pp.load_phoneme_list(os.path.join(cfg["output"]["save_dir"], "phonemes.txt"))
    try:
        start = start_bigram(labels, a.init)
    except ValueError as err:
        ap.error(str(err))
    paths = find_audio(a.audio)
    if not paths:
        ap.error("no audio file found")
    lang_id = None if a.lang_id is None or a.lang_id < 0 else a.lang_id
    from .infer import Labeler
    lab = Labeler(a.config, a.checkpoint, a.device)

    def report(k, r):
        print(f"round {k}: {r.files} files, {r.frames} frames, {r.successions:.1f} expected successions, "
              f"{r.nats_per_frame:.9f} nats per frame", flush=True)
    try:
        bg, rounds = adapt(lab, paths, start, a.iterations, a.prior_count, a.smoothing, weight, penalty, lang_id, threshold,
                           use_prior=bool(a.init), verbose=False, report=report)
    except ValueError as err:
        ap.error(str(err))
    PH.save(bg, a.output)
    print(f"{len(paths)} audio files, {a.iterations} rounds, {len(bg.symbols) - 1} phonemes -> {a.output}")


if __name__ == "__main__":
    main()
