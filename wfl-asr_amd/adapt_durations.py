"""Learn the phoneme duration prior of the Viterbi alignment (`postprocess.duration_prior`) from audio and transcripts alone: EM
re-estimation over the explicit-duration lattice the search runs on.

durations.estimate counts run lengths in timed `.lab` files.  Who runs a forced aligner has recordings and `.txt` transcripts and wants
such files: timed labels are what they lack.  One EM round here forwards the audio, lets the GPU sum, over every alignment of a file's
transcript weighted by its probability, how long every token lasts (Labeler.expected_durations, align.duration_prior_expected_counts,
wfl_align_duration_prior_counts), adds those length posteriors up per phoneme, and turns the expected counts into a prior exactly as
estimate turns its integer counts into one (durations.reestimate).  The result is a phoneme_durations.json like any other.

  adapt   the loop: start prior -> [expected_durations, reestimate] x iterations -> (DurationPrior, one record per round)
  python -m wfl_asr_amd.adapt_durations AUDIO... -ckpt best_model.pt -c config.yaml -o phoneme_durations.json
         [--init phoneme_durations.json] [--iterations K=3] [--max-frames D=32] [--prior-count M=0] [--smoothing S=0.1]
         [--duration-prior-weight W] [--lang-id ID] [--confidence-threshold T]

Transcripts are the `{audio}.txt` files infer.py reads.  Every round forwards the audio again; the logits are not kept between rounds
(DESIGN.md section 8).
"""
from __future__ import annotations

from typing import List, NamedTuple

from . import durations as DU
from .adapt_bigram import find_audio


class Round(NamedTuple):
    files: int              # files that were counted
    frames: int
    tokens: int
    nats_per_frame: float   # sum logZ / frames: the log mass the transcripts' alignments and the prior keep, per frame
    skipped: List[str]


def start_prior(init_path, max_frames, frame_duration) -> DU.DurationPrior:
    """The --init file, checked as far as it can be without the label set: its frame duration is the model's, and its D is the one
    asked for where one was asked for (ValueError otherwise).  None without a file."""
    if init_path is None:
        return None
    prior = DU.load(init_path)
    DU.check(prior, prior.phonemes, frame_duration, path=str(init_path))
    if max_frames is not None and int(max_frames) != int(prior.max_frames):
        raise ValueError(f"{init_path}: max_frames is {prior.max_frames}, --max-frames asks for {int(max_frames)}; the --init file fixes D")
    return prior


def adapt(labeler, audio_paths, transcripts, start: DU.DurationPrior, iterations=3, prior_count=0.0, smoothing=0.1, weight=1.0,
          lang_id=None, confidence_threshold=0.0, use_prior=False, verbose=True, report=None):
    """The EM loop -> (DurationPrior, [Round]).  start: the --init prior or durations.flat; it is also the prior of every
    re-estimation when use_prior (an --init file was given).  report(round number, Round) is called after every round."""
    prior, rounds = start, []
    for k in range(int(iterations)):
        counts, logz, frames, tokens, skipped = labeler.expected_durations(audio_paths, transcripts, prior, weight, lang_id,
                                                                           confidence_threshold, verbose)
        rec = Round(len(audio_paths) - len(skipped), frames, tokens, logz / max(frames, 1), list(skipped))
        rounds.append(rec)
        if report is not None:
            report(k + 1, rec)
        prior = DU.reestimate(counts, start.phonemes, start.max_frames, start if use_prior else None, prior_count, smoothing,
                              start.frame_duration)
    return prior, rounds


def main(argv=None):
    import argparse
    import os
    ap = argparse.ArgumentParser(
        prog="python -m wfl_asr_amd.adapt_durations",
        description="Re-estimate the phoneme duration prior of --align viterbi on audio with transcripts and no timed labels (EM over the "
                    "explicit-duration lattice of the search, on the GPU). Prints one line per round: files, frames, tokens and "
                    "sum logZ / frames in nats per frame. With --duration-prior-weight 1, --smoothing 0 and --prior-count 0 that figure "
                    "cannot decrease from round to round (the EM bound); with any other setting it is informative only.")
    ap.add_argument("audio", nargs="+", metavar="AUDIO", help="audio files, or folders whose *.wav files are taken; the transcript of "
                                                              "x.wav is x.txt")
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
    ap.add_argument("--duration-prior-weight", type=float, default=None, help="default: config postprocess.duration_prior_weight, else 1")
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
    from .infer import _read_forced, frame_duration, load_config
    try:
        init = start_prior(a.init, a.max_frames, frame_duration)
    except (ValueError, OSError) as err:
        ap.error(str(err))
    if not os.path.isfile(a.config):
        ap.error(f"config file not found: {a.config}")
    cfg = load_config(a.config)
    post = cfg.get("postprocess") or {}
    weight = post.get("duration_prior_weight") if a.duration_prior_weight is None else a.duration_prior_weight
    weight = 1.0 if weight is None else float(weight)
    threshold = float(post.get("confidence_threshold", 0.0) if a.confidence_threshold is None else a.confidence_threshold)
    if not weight >= 0.0 or not threshold >= 0.0:
        ap.error("--duration-prior-weight and --confidence-threshold must be >= 0")
    paths = find_audio(a.audio)
    if not paths:
        ap.error("no audio file found")
    transcripts = [_read_forced(p, False) for p in paths]
    if not any(transcripts):
        ap.error("no transcript found (the transcript of x.wav is x.txt)")
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
        print(f"round {k}: {r.files} files, {r.frames} frames, {r.tokens} tokens, {r.nats_per_frame:.9f} nats per frame", flush=True)
    try:
        prior, rounds = adapt(lab, paths, transcripts, start, a.iterations, a.prior_count, a.smoothing, weight, lang_id, threshold,
                              use_prior=init is not None, verbose=False, report=report)
    except ValueError as err:
        ap.error(str(err))
    DU.save(prior, a.output)
    empty = [p for p, r in zip(prior.phonemes, prior.log_prob) if r is None]
    if empty:
        print(f"in no transcript, no prior: {', '.join(empty)}")
    print(f"{len(paths)} audio files, {a.iterations} rounds, {len(prior.phonemes) - len(empty)} phonemes with a prior -> {a.output}")


if __name__ == "__main__":
    main()
