"""Learn the duration prior of the free decode (`postprocess.decode_duration_prior`) from audio WITHOUT labels or transcripts: EM
re-estimation over the explicit-duration BIO grammar the search runs on.

durations.estimate needs timed `.lab` files and adapt_durations needs `{audio}.txt` transcripts.  Who uses the free decode has neither:
a checkpoint and recordings of a new singer.  One EM round here forwards the audio, lets the GPU sum, over every legal path weighted by
its probability, how many runs of every phoneme last 1, 2, ... frames (Labeler.expected_free_durations,
decode.duration_expected_counts, wfl_decode_duration_counts), and turns the expected counts into a prior exactly as estimate turns its
integer counts into one (durations.reestimate).  The same pass yields the expected successions on the lattice that carries both
tables, so with --bigram-output the phone bigram is re-estimated under the duration prior in the same round (phonotactics.reestimate),
which adapt_bigram cannot do.  The results are a phoneme_durations.json and a phoneme_bigram.json like any other.

  adapt   the loop: start prior -> [expected_free_durations, reestimate] x iterations -> (DurationPrior, Bigram or None, [Round])
  python -m wfl_asr_amd.adapt_decode_durations AUDIO... -ckpt best_model.pt -c config.yaml -o phoneme_durations.json
         [--init phoneme_durations.json] [--iterations K=3] [--max-frames D=32] [--prior-count M=0] [--smoothing S=0.1]
         [--decode-duration-prior-weight W] [--phoneme-bigram PATH] [--bigram-weight W] [--switch-penalty L]
         [--bigram-output PATH] [--lang-id ID] [--confidence-threshold T]

Every round forwards the audio again; the logits are not kept between rounds.
"""
from __future__ import annotations

import os
from typing import List, NamedTuple

import numpy as np

from . import durations as DU
from . import phonotactics as PH
from .adapt_bigram import find_audio, start_bigram
from .adapt_durations import start_prior
from .decode import class_table


class Round(NamedTuple):
    files: int              # files that were counted
    frames: int
    runs: float             # the expected number of phoneme runs, all files
    nats_per_frame: float   # (sum logZ - sum lse) / frames: the log mass the grammar and the two tables keep, per frame
    skipped: List[str]


def adapt(labeler, audio_paths, start: DU.DurationPrior, iterations=3, prior_count=0.0, smoothing=0.1, weight=1.0, bigram=None,
          bigram_weight=1.0, switch_penalty=0.0, adapt_bigram=False, bigram_is_prior=False, lang_id=None, confidence_threshold=0.0,
          use_prior=False, verbose=True, report=None):
    """The EM loop -> (DurationPrior, Bigram or None, [Round]).  start: the --init prior or durations.flat; it is also the prior of
    every re-estimation when use_prior (an --init file was given).  bigram: the grammar's phonotactics.Bigram in the symbols' order
    (adapt_bigram.start_bigram), or None: the flat table -switch_penalty.  adapt_bigram: re-estimate `bigram` (not None then) from
    the same round's expected successions; otherwise it stays what it is.  bigram_is_prior: `bigram` came from a file, and what it
    forbids stays forbidden (phonotactics.reestimate's prior, with no pseudo-counts).  report(round number, Round) is called after
    every round."""
    ct = class_table(labeler.labels)
    prior, bg, rounds = start, bigram, []
    for k in range(int(iterations)):
        trans = None if bg is None else PH.transition_table(bg, ct, labeler.labels, switch_penalty, bigram_weight)
        if trans is None:
            n = len(ct.pairs) + 1
            trans = np.full((n, n), -float(switch_penalty), np.float32)
        counts, succ, logz, lse, frames, skipped = labeler.expected_free_durations(audio_paths, trans, prior, weight, lang_id,
                                                                                   confidence_threshold, verbose)
        D = int(start.max_frames)
        rec = Round(len(audio_paths) - len(skipped), frames, float(counts[:, :D].sum()), (logz - lse) / max(frames, 1), list(skipped))
        rounds.append(rec)
        if report is not None:
            report(k + 1, rec)
        prior = DU.reestimate(counts, start.phonemes, start.max_frames, start if use_prior else None, prior_count, smoothing,
                              start.frame_duration)
        if adapt_bigram:
            bg = PH.reestimate(succ, bigram.symbols, bigram if bigram_is_prior else None, 0.0, smoothing)
    return prior, (bg if adapt_bigram else None), rounds


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(
        prog="python -m wfl_asr_amd.adapt_decode_durations",
        description="Re-estimate the duration prior of --decode viterbi (postprocess.decode_duration_prior) on audio without labels or "
                    "transcripts (EM over the explicit-duration grammar of the search, on the GPU). Prints one line per round: files, "
                    "frames, expected runs and (sum logZ - sum lse) / frames in nats per frame. With --decode-duration-prior-weight 1, "
                    "--bigram-weight 1, --switch-penalty 0, --smoothing 0 and --prior-count 0 that figure cannot decrease from round to "
                    "round (the EM bound); with any other setting it is informative only.")
    ap.add_argument("audio", nargs="+", metavar="AUDIO", help="audio files, or folders whose *.wav files are taken")
    ap.add_argument("-ckpt", "--checkpoint", required=True, help="the model checkpoint")
    ap.add_argument("-c", "--config", required=True, help="the model's config.yaml")
    ap.add_argument("-o", "--output", required=True, help="the phoneme_durations.json to write")
    ap.add_argument("--init", help="a phoneme_durations.json to start from; it fixes D, it is also the prior of every round, and what it "
                                   "forbids stays forbidden (default: a flat prior that forbids nothing)")
    ap.add_argument("--iterations", type=int, default=3, help="EM rounds; every round forwards the audio again (default 3)")
    ap.add_argument("--max-frames", type=int, default=None, help="D: durations up to D frames get a histogram entry, longer ones a "
                                                                 "geometric tail (default 32, or what --init holds)")
    ap.add_argument("--prior-count", type=float, default=0.0, help="pseudo-runs per phoneme taken from --init (default 0)")
    ap.add_argument("--smoothing", type=float, default=0.1, help="added to every allowed expected count (default 0.1)")
    ap.add_argument("--decode-duration-prior-weight", type=float, default=None,
                    help="default: config postprocess.decode_duration_prior_weight, else 1")
    ap.add_argument("--phoneme-bigram", default=None, help="the grammar's phoneme_bigram.json (default: config postprocess.phoneme_bigram; "
                                                           "without one the flat switch penalty)")
    ap.add_argument("--bigram-weight", type=float, default=None, help="default: config postprocess.bigram_weight, else 1")
    ap.add_argument("--switch-penalty", type=float, default=None, help="default: config postprocess.switch_penalty, else 0")
    ap.add_argument("--bigram-output", default=None, help="also re-estimate the phone bigram, under the duration prior, from the same "
                                                          "rounds' expected successions, and write it here (it starts from "
                                                          "--phoneme-bigram, else from every succession equally likely)")
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
    if a.max_frames is not None and not 1 <= a.max_frames <= DU.MAX_FRAMES:
        ap.error(f"--max-frames must be 1 .. {DU.MAX_FRAMES}")
    from . import postprocess as pp
    from .infer import frame_duration, load_config
    try:
        init = start_prior(a.init, a.max_frames, frame_duration)
    except (ValueError, OSError) as err:
        ap.error(str(err))
    if not os.path.isfile(a.config):
        ap.error(f"config file not found: {a.config}")
    cfg = load_config(a.config)
    post = cfg.get("postprocess") or {}

    def setting(given, key, default):
        v = post.get(key) if given is None else given
        return default if v is None else float(v)
    weight = setting(a.decode_duration_prior_weight, "decode_duration_prior_weight", 1.0)
    bigram_weight = setting(a.bigram_weight, "bigram_weight", 1.0)
    penalty = setting(a.switch_penalty, "switch_penalty", 0.0)
    threshold = setting(a.confidence_threshold, "confidence_threshold", 0.0)
    if not weight >= 0.0 or not bigram_weight >= 0.0 or not penalty >= 0.0 or not threshold >= 0.0:
        ap.error("--decode-duration-prior-weight, --bigram-weight, --switch-penalty and --confidence-threshold must be >= 0")
    bigram_path = a.phoneme_bigram if a.phoneme_bigram is not None else post.get("phoneme_bigram")
    labels = pp.load_phoneme_list(os.path.join(cfg["output"]["save_dir"], "phonemes.txt"))
    try:
        bigram = start_bigram(labels, bigram_path) if (bigram_path or a.bigram_output) else None     # (also the symbol cap's check)
        if bigram is None:
            start_bigram(labels, None)
    except (ValueError, OSError) as err:
        ap.error(str(err))
    paths = find_audio(a.audio)
    if not paths:
        ap.error("no audio file found")
    lang_id = None if a.lang_id is None or a.lang_id < 0 else a.lang_id
    from .infer import Labeler
    lab = Labeler(a.config, a.checkpoint, a.device)
    names = lab._names_for(lab._lang_name(lang_id))[1]
    try:
        if init is not None:
            DU.check(init, names, frame_duration, path=str(a.init))      # before any forward
        start = init if init is not None else DU.flat(names, 32 if a.max_frames is None else a.max_frames, frame_duration)
    except ValueError as err:
        ap.error(str(err))

    def report(k, r):
        print(f"round {k}: {r.files} files, {r.frames} frames, {r.runs:.1f} runs, {r.nats_per_frame:.9f} nats per frame", flush=True)
    try:
        prior, bg, rounds = adapt(lab, paths, start, a.iterations, a.prior_count, a.smoothing, weight, bigram, bigram_weight, penalty,
                                  adapt_bigram=bool(a.bigram_output), bigram_is_prior=bool(bigram_path), lang_id=lang_id, confidence_threshold=threshold,
                                  use_prior=init is not None, verbose=False, report=report)
    except ValueError as err:
        ap.error(str(err))
    DU.save(prior, a.output)
    if bg is not None:
        PH.save(bg, a.bigram_output)
    empty = [p for p, r in zip(prior.phonemes, prior.log_prob) if r is None]
    if empty:
        print(f"in no expected run, no prior: {', '.join(empty)}")
    print(f"{len(paths)} audio files, {a.iterations} rounds, {len(prior.phonemes) - len(empty)} phonemes with a prior -> {a.output}"
          + (f", bigram -> {a.bigram_output}" if bg is not None else ""))


if __name__ == "__main__":
    main()
