"""BIO-grammar Viterbi decode of files WITHOUT a transcript over the model's frame logits (`postprocess.decode: viterbi`).

The reference's free decode takes each frame's argmax on its own, turns frames below `confidence_threshold` into `O`, runs a median
filter over the integer class ids and lets `decode_bio_tags` make what it can of the tag string (infer.py:86-96, 164-174, 293-302;
utils.py:47-61).  That decode knows nothing of the grammar: `I-x` straight after `B-y` or `O` silently opens a segment, a one-frame
flicker between two near-tied classes cuts a phoneme in three, and the posteriors are thrown away first.  This module instead
searches the frame logits for the best LEGAL tag string (csrc/decode.hip, include/wfl_asr.h `wfl_decode`): every `I-p` directly
follows `B-p` or `I-p`, and every run that is opened costs `switch_penalty` nats.

  class_table         label set -> (O class, (B class, I class or -1) per phoneme); every other class is never chosen
  bio_viterbi         the C ABI on CUDA tensors: a ragged batch of clips in one call
  bio_viterbi_bigram  the same search with a phone-bigram prior: a table of transition weights per (previous symbol, opened symbol)
                      in place of the flat switch penalty (csrc/decode_bigram.hip, `wfl_decode_bigram`; phonotactics.py makes the table)
  bio_viterbi_duration  the bigram search with a duration prior per phoneme: an explicit-duration (semi-Markov) search
                      (csrc/decode_duration.hip, `wfl_decode_duration`; durations.py makes the table, duration_symbol_rows the rows)
  decode_posteriors   forward-backward over the same grammar (csrc/decode_posterior.hip, `wfl_decode_posterior`): logZ, and per frame
                      the posterior of the phoneme and of the exact class the path chose (`postprocess.decode_scores`)
  decode_posteriors_bigram  the same over the grammar of bio_viterbi_bigram, the table included (csrc/decode_bigram_posterior.hip,
                      `wfl_decode_bigram_posterior`; `postprocess.bigram_scores`)
  decode_posteriors_duration  the same over the explicit-duration grammar of bio_viterbi_duration, the table and the duration prior
                      included (csrc/decode_duration_posterior.hip, `wfl_decode_duration_posterior`; `postprocess.decode_duration_scores`)
  bigram_expected_counts  the expected successions of a batch of clips under bio_viterbi_bigram's path distribution, one [N, N] table
                      per clip (csrc/decode_bigram_counts.hip, `wfl_decode_bigram_counts`): the E-step of adapt_bigram.py
  duration_expected_counts  the expected run lengths [phonemes, D + 1] and successions [N, N] per clip under bio_viterbi_duration's
                      path distribution (csrc/decode_duration_counts.hip, `wfl_decode_duration_counts`): the E-step of
                      adapt_decode_durations.py
  path_segments_free  the path's ids of a file, chunk by chunk, -> segments; a run that crosses a chunk seam is one segment
  free_score          those outputs + bio_viterbi's score -> FreeScore / RunScore records, run j being segment j of the path
"""
from __future__ import annotations

import ctypes as C
from typing import List, NamedTuple

import numpy as np
import torch

from . import _lib
from . import native_post as npost
from ._lib import back_to_back, host_ptr as _hp, ptr as _ptr
from .align import class_pairs
from .options import DECODE_MODES  # noqa: F401  (decode.DECODE_MODES stays importable)

MAX_CLASSES = 1024         # wfl_decode's class cap (status 2 above it)
MAX_BIGRAM_SYMBOLS = 192   # wfl_decode_bigram's symbol cap, O + 191 phonemes (WFL_DECODE_BIGRAM_MAX_SYMBOLS; status 2 above it)
STATUS_OK, STATUS_OVER_CAP, STATUS_BAD_CLASS = 0, 2, 4
STATUS_NOT_A_PATH = 8      # the posterior entries alone: `ids` is not a path of the grammar


class ClassTable(NamedTuple):
    o_id: int
    pairs: np.ndarray      # [phonemes, 2] int32: B class, I class or -1


def class_table(label_list) -> ClassTable:
    """The roles wfl_decode needs from a label set: the `O` class and, per phoneme that has a `B-` class, (B class, I class or -1),
    in the order of the B classes.  An `I-p` without `B-p` and a name that is neither `O`, `B-...` nor `I-...` get no entry: the
    search never chooses them."""
    if "O" not in label_list:
        raise ValueError("the label set has no 'O' class")
    both = class_pairs(label_list)
    b_only = {tag[2:]: c for c, tag in enumerate(label_list) if tag.startswith("B-") and tag[2:] not in both}
    pairs = sorted(list(both.values()) + [(c, -1) for c in b_only.values()])
    return ClassTable(label_list.index("O"), np.array(pairs, np.int32).reshape(-1, 2))


def _workspace_bytes(symbol, n_frames, n_pairs, *more) -> int:
    """`more`: what the entry's size function takes after n_pairs (wfl_decode_duration's D)."""
    T = np.ascontiguousarray(n_frames, np.int32)
    n = int(getattr(_lib.load(), symbol)(_hp(T), T.size, int(n_pairs), *more))
    if n < 0:
        raise _lib.WflError(f"{symbol}: negative frame or pair count" + (f", or a bad {more!r}" if more else ""))
    return n


def workspace_bytes(n_frames, n_pairs) -> int:
    return _workspace_bytes("wfl_decode_workspace_bytes", n_frames, n_pairs)


def bigram_workspace_bytes(n_frames, n_pairs) -> int:
    return _workspace_bytes("wfl_decode_bigram_workspace_bytes", n_frames, n_pairs)


def posterior_workspace_bytes(n_frames, n_pairs) -> int:
    return _workspace_bytes("wfl_decode_posterior_workspace_bytes", n_frames, n_pairs)


def bigram_posterior_workspace_bytes(n_frames, n_pairs) -> int:
    return _workspace_bytes("wfl_decode_bigram_posterior_workspace_bytes", n_frames, n_pairs)


def bigram_counts_workspace_bytes(n_frames, n_pairs) -> int:
    return _workspace_bytes("wfl_decode_bigram_counts_workspace_bytes", n_frames, n_pairs)


def duration_workspace_bytes(n_frames, n_pairs, D) -> int:
    return _workspace_bytes("wfl_decode_duration_workspace_bytes", n_frames, n_pairs, int(D))


def duration_posterior_workspace_bytes(n_frames, n_pairs, D) -> int:
    return _workspace_bytes("wfl_decode_duration_posterior_workspace_bytes", n_frames, n_pairs, int(D))


def duration_counts_workspace_bytes(n_frames, n_pairs, D) -> int:
    return _workspace_bytes("wfl_decode_duration_counts_workspace_bytes", n_frames, n_pairs, int(D))


def _check_clips(logits, n_frames, table, switch_penalty, threshold, frame_offsets):
    """The validation the three entries share -> (o_id, pairs, nb, T, F0), _call's clip arguments."""
    if not logits.is_cuda or logits.dim() != 2 or logits.dtype != torch.float32 or (logits.numel() and logits.stride(1) != 1):
        raise ValueError("logits must be a [rows, C] float32 CUDA tensor with contiguous rows")
    o_id, pairs = table
    pairs = np.ascontiguousarray(np.asarray(pairs, np.int32).reshape(-1, 2))
    if not 0 <= int(o_id) < logits.shape[1]:
        raise ValueError(f"o_id {o_id} is not a class of the logits ({logits.shape[1]} columns)")
    if not float(switch_penalty) >= 0.0:
        raise ValueError(f"switch_penalty must be >= 0, got {switch_penalty!r}")
    if not float(threshold) >= 0.0:
        raise ValueError(f"threshold must be >= 0, got {threshold!r}")
    nb = len(n_frames)
    T = np.ascontiguousarray(np.asarray(n_frames, np.int32).reshape(nb))
    if nb and int(T.min()) < 0:
        raise ValueError("a clip has a negative frame count")
    if frame_offsets is None:
        frame_offsets = back_to_back(T)
    F0 = np.ascontiguousarray(frame_offsets, np.int64).reshape(nb)
    if nb and (int(F0.min()) < 0 or int((F0 + T).max()) > logits.shape[0]):
        raise ValueError("a clip's frames run past the logits rows")
    return int(o_id), pairs, nb, T, F0


def _call(entry, logits, clips, middle, outputs, stream, ws_more=()):
    """What the three entries share after _check_clips (`clips`: its result): `entry`'s workspace, the class pairs on the device, the
    call on `stream` (default: the current one) and its check.  middle: the arguments between n_pairs and the workspace, outputs: the
    tensors after it; a float or an int goes as it is, a tensor as its pointer, a numpy array is uploaded for the call.  ws_more: what
    the entry's size function takes after n_pairs."""
    o_id, pairs, nb, T, F0 = clips
    lib = _lib.load()
    dev = logits.device
    ws_n = _workspace_bytes(entry + "_workspace_bytes", T, len(pairs), *ws_more) if logits.shape[1] <= MAX_CLASSES else 0
    ws = torch.empty(max(ws_n, 1), dtype=torch.uint8, device=dev)
    d_pairs = torch.from_numpy(pairs if len(pairs) else np.full((1, 2), -1, np.int32)).to(dev)
    temporaries = [ws, d_pairs]
    args = []
    for m in middle:
        if isinstance(m, np.ndarray):
            m = torch.from_numpy(m).to(dev)
            temporaries.append(m)
        args.append(_ptr(m) if isinstance(m, torch.Tensor) else m)
    with torch.cuda.device(dev):
        st = stream if stream is not None else torch.cuda.current_stream(dev)
        ldl = logits.stride(0) if logits.numel() else logits.shape[1]      # (an empty tensor's strides say nothing)
        rc = getattr(lib, entry)(_ptr(logits), ldl, logits.shape[1], o_id, _hp(F0), _hp(T), nb, _ptr(d_pairs), len(pairs), *args,
                                 _ptr(ws), ws_n, *(_ptr(t) for t in outputs), C.c_void_p(st.cuda_stream))
        _lib.check(rc, entry)
        for t in temporaries:
            t.record_stream(st)


def bio_viterbi(logits, n_frames, table, switch_penalty, threshold, frame_offsets=None, stream=None):
    """BIO-grammar Viterbi decode of a ragged batch of clips on the GPU.

    logits          [rows, C] float32 CUDA tensor (rows contiguous in C; clip b = rows frame_offsets[b] .. + n_frames[b]).  With
                    `lang_id=None` these are the language-averaged logits the forward returns, and the search runs on those.
    n_frames        frames per clip (host ints)
    table           class_table(label_list), or any (o_id, [(B class, I class or -1), ...])
    switch_penalty  lambda >= 0, nats per opened run
    threshold       a frame whose largest softmax probability is below it can only be O (0: no frame is forced)
    frame_offsets   first row of each clip (default: the clips back to back)
    -> (ids [rows] int32, score [clips] float32, status [clips] int32), CUDA tensors on `stream`'s device.  A clip with status != 0
    (STATUS_OVER_CAP: C > 1024; STATUS_BAD_CLASS: a class of the table out of range or used twice) is O everywhere, score 0."""
    clips = _check_clips(logits, n_frames, table, switch_penalty, threshold, frame_offsets)
    nb = clips[2]
    ids = torch.empty(logits.shape[0], dtype=torch.int32, device=logits.device)
    score = torch.empty(max(nb, 1), dtype=torch.float32, device=logits.device)
    status = torch.empty(max(nb, 1), dtype=torch.int32, device=logits.device)
    _call("wfl_decode", logits, clips, (float(switch_penalty), float(threshold)), (ids, score, status), stream)
    return ids, score[:nb], status[:nb]


def check_transitions(trans, n_pairs) -> np.ndarray:
    """A table of transition weights for bio_viterbi_bigram -> contiguous float32 [n_pairs + 1, n_pairs + 1].  Symbol 0 is O, symbol
    1 + p is phoneme p of the class table; rows are the previous symbol.  Entries are finite or -inf (a forbidden succession): never
    NaN, never +inf, and every [p][O] finite, so every clip has a path (a forced frame can only be O); [O][O] is never read and not
    checked."""
    if isinstance(trans, torch.Tensor):
        trans = trans.detach().cpu().numpy()
    w = np.asarray(trans)
    n = int(n_pairs) + 1
    if w.dtype != np.float32:
        raise ValueError(f"trans must be float32, got {w.dtype}")
    if w.shape != (n, n):
        raise ValueError(f"trans must be a [{n}, {n}] table (O and the {n - 1} phonemes of the class table), got {list(w.shape)}")
    w = np.array(w, np.float32, order="C")            # (a copy)
    w[0, 0] = 0.0                                     # [O][O] is never read (O after O costs nothing): whatever it holds is fine
    if np.isnan(w).any():
        raise ValueError("trans holds a NaN")
    if np.isposinf(w).any():
        raise ValueError("trans holds +inf (entries are finite, or -inf for a forbidden succession)")
    if not np.isfinite(w[:, 0]).all():
        raise ValueError("every trans[p][O] must be finite: a frame forced to O needs a way in")
    return w


def bio_viterbi_bigram(logits, n_frames, table, trans, threshold, frame_offsets=None, stream=None):
    """bio_viterbi with a phone-bigram prior: every opened run costs trans[previous symbol][opened symbol] (natural-log weights, <= 0
    for a prior) instead of one flat switch penalty.  Arguments and results are bio_viterbi's, but:

    trans  float32 [n + 1, n + 1] over O (symbol 0) and the n phonemes of `table` in its order (check_transitions;
           phonotactics.transition_table builds it from a phoneme_bigram.json); -inf forbids a succession.
    A label set with more than 191 phonemes is over the kernel's cap (MAX_BIGRAM_SYMBOLS): STATUS_OVER_CAP, O everywhere, score 0."""
    clips = _check_clips(logits, n_frames, table, 0.0, threshold, frame_offsets)
    w = check_transitions(trans, len(clips[1]))
    nb = clips[2]
    ids = torch.empty(logits.shape[0], dtype=torch.int32, device=logits.device)
    score = torch.empty(max(nb, 1), dtype=torch.float32, device=logits.device)
    status = torch.empty(max(nb, 1), dtype=torch.int32, device=logits.device)
    _call("wfl_decode_bigram", logits, clips, (w, float(threshold)), (ids, score, status), stream)
    return ids, score[:nb], status[:nb]


MAX_DURATION = 32          # wfl_decode_duration's longest explicit duration D (wfl_align_duration_prior's)


def check_duration_table(dur) -> np.ndarray:
    """A table of run-length scores for bio_viterbi_duration -> contiguous float32 [rows, D + 1], 1 <= D <= 32: columns L(1) .. L(D), then
    the per-frame tail (durations.table builds it).  Entries are finite or -inf (a forbidden duration): never NaN, never +inf; a tail is
    <= 0 or -inf."""
    if isinstance(dur, torch.Tensor):
        dur = dur.detach().cpu().numpy()
    d = np.asarray(dur)
    if d.dtype != np.float32:
        raise ValueError(f"dur must be float32, got {d.dtype}")
    if d.ndim != 2 or not 2 <= d.shape[1] <= MAX_DURATION + 1:
        raise ValueError(f"dur must be a [rows, D + 1] table with 1 <= D <= {MAX_DURATION}, got {list(d.shape)}")
    if np.isnan(d).any():
        raise ValueError("dur holds a NaN")
    if np.isposinf(d).any():
        raise ValueError("dur holds +inf (entries are finite, or -inf for a forbidden duration)")
    if (d[:, -1] > 0).any():
        raise ValueError("a tail of dur is > 0 (the last column is the per-frame score past D frames: <= 0 or -inf)")
    return np.ascontiguousarray(d)


def check_symbol_rows(sym_dur, n_pairs, rows) -> np.ndarray:
    """The phonemes' rows of the duration table for bio_viterbi_duration -> contiguous int32 [n_pairs], every entry in -1 .. rows - 1."""
    if isinstance(sym_dur, torch.Tensor):
        sym_dur = sym_dur.detach().cpu().numpy()
    r = np.asarray(sym_dur)
    if r.dtype != np.int32:
        raise ValueError(f"sym_dur must be int32, got {r.dtype}")
    if r.shape != (int(n_pairs),):
        raise ValueError(f"sym_dur must hold one row per phoneme of the class table ([{int(n_pairs)}]), got {list(r.shape)}")
    if r.size and (int(r.min()) < -1 or int(r.max()) >= int(rows)):
        raise ValueError(f"sym_dur must lie in -1 .. {int(rows) - 1} (the rows of dur; -1: no prior)")
    return np.ascontiguousarray(r)


def bio_viterbi_duration(logits, n_frames, table, trans, dur, sym_dur, threshold, frame_offsets=None, stream=None):
    """bio_viterbi_bigram with a duration prior per phoneme: an explicit-duration (semi-Markov) search (csrc/decode_duration.hip,
    `wfl_decode_duration`).  A run of d frames of phoneme p adds L(d) of row sym_dur[p] of `dur`.  Arguments and results are
    bio_viterbi_bigram's, but:

    dur      float32 [rows, D + 1], 1 <= D <= 32: L(1) .. L(D), then the per-frame tail of every frame past D (check_duration_table;
             durations.table builds it from a duration prior); -inf forbids a duration.
    sym_dur  int32 [phonemes of `table`]: each phoneme's row of `dur`, -1 for no prior (duration_symbol_rows).
    O runs carry no prior.  With every sym_dur = -1, or an all-zero `dur`, the objective is bio_viterbi_bigram's."""
    clips = _check_clips(logits, n_frames, table, 0.0, threshold, frame_offsets)
    w = check_transitions(trans, len(clips[1]))
    d = check_duration_table(dur)
    r = check_symbol_rows(sym_dur, len(clips[1]), d.shape[0])
    nb = clips[2]
    ids = torch.empty(logits.shape[0], dtype=torch.int32, device=logits.device)
    score = torch.empty(max(nb, 1), dtype=torch.float32, device=logits.device)
    status = torch.empty(max(nb, 1), dtype=torch.int32, device=logits.device)
    D = d.shape[1] - 1
    r_up = r if r.size else np.full(1, -1, np.int32)
    d_up = d if d.size else np.zeros((1, D + 1), np.float32)
    _call("wfl_decode_duration", logits, clips, (w, r_up, d_up, int(d.shape[0]), D, float(threshold)), (ids, score, status), stream,
          ws_more=(D,))
    return ids, score[:nb], status[:nb]


def duration_symbol_rows(prior, table, labels, output_names=None) -> np.ndarray:
    """The sym_dur of bio_viterbi_duration: for each phoneme of the class table `table` (class_table(labels)) the row of the duration
    prior `prior` (durations.DurationPrior) that its OUTPUT name has -- the naming rule of align.duration_rows, whose tokens are output
    names.  output_names: a mapping from a phoneme's label name (the `x` of `B-x`) to the name it is written under (the merge map's
    back-mapping); None, or a name it lacks: the label name itself.  Two phonemes with one output name share its row.  A name the
    prior lacks, or whose row is null (no sample), gives -1: no prior."""
    row = {name: i for i, name in enumerate(prior.phonemes) if prior.log_prob[i] is not None}
    names = [str(labels[int(b)])[2:] for b, _ in np.asarray(table[1], np.int32).reshape(-1, 2)]
    out = output_names or {}
    return np.array([row.get(out.get(n, n), -1) for n in names], np.int32)


def decode_posteriors(logits, n_frames, table, switch_penalty, threshold, ids, frame_offsets=None, stream=None):
    """Forward-backward over the grammar of bio_viterbi, for the same ragged batch of clips (same arguments), given its `ids`.

    ids  [rows] int32 CUDA tensor: bio_viterbi's output for these clips (row frame_offsets[b] + t)
    -> (logz [clips], post [rows], cls_post [rows], status [clips]): float32 / int32 CUDA tensors.  logz: log of the summed weight
    exp(sum of the logits on the path - switch_penalty * runs opened) of every legal path; post: the posterior that the frame belongs
    to the phoneme the path gives it (B-p or I-p; to O on an O frame), in [0, 1]; cls_post: the posterior of the exact class, so on a
    run's first frame that the run opens exactly there; cls_post <= post.  Rows outside the clips are not written.  A clip with
    status != 0 gets zeros (STATUS_NOT_A_PATH: `ids` is not a legal path of these clips)."""
    clips = _check_clips(logits, n_frames, table, switch_penalty, threshold, frame_offsets)
    return _posteriors("wfl_decode_posterior", logits, clips, (float(switch_penalty), float(threshold)), ids, stream)


def _posteriors(entry, logits, clips, middle, ids, stream, ws_more=()):
    """What the posterior entries share after their own checks: the check of `ids`, the outputs and the call.  ws_more: _call's."""
    dev = logits.device
    if not isinstance(ids, torch.Tensor) or not ids.is_cuda or ids.device != dev or ids.dtype != torch.int32 or ids.dim() != 1 \
            or (ids.numel() and ids.stride(0) != 1) or ids.shape[0] != logits.shape[0]:
        raise ValueError("ids must be bio_viterbi's [rows] int32 CUDA tensor for these logits")
    nb, rows = clips[2], logits.shape[0]
    per_frame = torch.empty((2, max(rows, 1)), dtype=torch.float32, device=dev)
    logz = torch.empty(max(nb, 1), dtype=torch.float32, device=dev)
    status = torch.empty(max(nb, 1), dtype=torch.int32, device=dev)
    _call(entry, logits, clips, (*middle, ids), (logz, per_frame[0], per_frame[1], status), stream, ws_more=ws_more)
    return logz[:nb], per_frame[0, :rows], per_frame[1, :rows], status[:nb]


def decode_posteriors_bigram(logits, n_frames, table, trans, threshold, ids, frame_offsets=None, stream=None):
    """Forward-backward over the grammar of bio_viterbi_bigram, for the same ragged batch of clips (same arguments), given its `ids`:
    decode_posteriors with the table `trans` (check_transitions) in place of the flat switch penalty.

    -> (logz [clips], post [rows], cls_post [rows], status [clips]) as decode_posteriors; logz is the log of the summed weight
    exp(sum of the logits on the path + sum of trans over the runs opened) of every legal path.  A clip with status != 0 gets zeros
    (STATUS_OVER_CAP also above MAX_BIGRAM_SYMBOLS; STATUS_NOT_A_PATH also for a run opened through a -inf entry of `trans`).  With
    trans identically -switch_penalty the results are decode_posteriors'."""
    clips = _check_clips(logits, n_frames, table, 0.0, threshold, frame_offsets)
    w = check_transitions(trans, len(clips[1]))
    return _posteriors("wfl_decode_bigram_posterior", logits, clips, (w, float(threshold)), ids, stream)


def decode_posteriors_duration(logits, n_frames, table, trans, dur, sym_dur, threshold, ids, frame_offsets=None, stream=None):
    """Forward-backward over the explicit-duration grammar of bio_viterbi_duration, for the same ragged batch of clips (same
    arguments), given its `ids`: decode_posteriors_bigram with the duration table `dur` (check_duration_table) and the phonemes' rows
    `sym_dur` (check_symbol_rows) beside the table `trans` (csrc/decode_duration_posterior.hip, `wfl_decode_duration_posterior`).

    -> (logz [clips], post [rows], cls_post [rows], status [clips]) as decode_posteriors; logz is the log of the summed weight
    exp(sum of the logits on the path + sum of trans over the runs opened + sum of L(d) over the phoneme runs) of every legal path.
    post: the posterior that the frame belongs to the path's phoneme at all; cls_post on a run's first frame: that a run opens exactly
    there.  A clip with status != 0 gets zeros (STATUS_OVER_CAP also above MAX_BIGRAM_SYMBOLS; STATUS_NOT_A_PATH also for a run
    opened through a -inf entry of `trans` and for a run whose length has L = -inf).  With every sym_dur = -1, or an all-zero `dur`,
    the results are decode_posteriors_bigram's."""
    clips = _check_clips(logits, n_frames, table, 0.0, threshold, frame_offsets)
    w = check_transitions(trans, len(clips[1]))
    d = check_duration_table(dur)
    r = check_symbol_rows(sym_dur, len(clips[1]), d.shape[0])
    D = d.shape[1] - 1
    r_up = r if r.size else np.full(1, -1, np.int32)
    d_up = d if d.size else np.zeros((1, D + 1), np.float32)
    return _posteriors("wfl_decode_duration_posterior", logits, clips, (w, r_up, d_up, int(d.shape[0]), D, float(threshold)), ids, stream,
                       ws_more=(D,))


def bigram_expected_counts(logits, n_frames, table, trans, threshold, frame_offsets=None, stream=None):
    """The expected successions of a ragged batch of clips under the grammar of bio_viterbi_bigram (same arguments): one Baum-Welch
    E-step over the table `trans` (check_transitions).

    -> (logz [clips] float32, counts [clips, N, N] float32, status [clips] int32), CUDA tensors; N = phonemes + 1, symbol 0 is O, rows
    are the PREVIOUS symbol.  counts[b][s][q] is the expected number of runs of q opened directly after s in clip b, the runs counted
    as the search counts them (every B-q frame, and every O frame whose predecessor is not O); [O][O] and every entry whose `trans` is
    -inf are exactly 0.  logz is decode_posteriors_bigram's.  A clip with status != 0 (STATUS_OVER_CAP also above MAX_BIGRAM_SYMBOLS;
    STATUS_BAD_CLASS) gets logz 0 and an all-zero table; so does an empty clip, with status 0."""
    clips = _check_clips(logits, n_frames, table, 0.0, threshold, frame_offsets)
    w = check_transitions(trans, len(clips[1]))
    nb, n = clips[2], len(clips[1]) + 1
    dev = logits.device
    logz = torch.empty(max(nb, 1), dtype=torch.float32, device=dev)
    counts = torch.empty((max(nb, 1), n, n), dtype=torch.float32, device=dev)
    status = torch.empty(max(nb, 1), dtype=torch.int32, device=dev)
    _call("wfl_decode_bigram_counts", logits, clips, (w, float(threshold)), (logz, counts, status), stream)
    return logz[:nb], counts[:nb], status[:nb]


def duration_expected_counts(logits, n_frames, table, trans, dur, sym_dur, threshold, frame_offsets=None, stream=None):
    """The expected run lengths and successions of a ragged batch of clips under the explicit-duration grammar of bio_viterbi_duration
    (same arguments): one E-step over the duration table `dur` and the table `trans` (csrc/decode_duration_counts.hip,
    `wfl_decode_duration_counts`).

    -> (logz [clips] float32, succ [clips, N, N] float32, dur_counts [clips, phonemes, D + 1] float32, status [clips] int32), CUDA
    tensors.  succ is bigram_expected_counts' table on this grammar (rows the PREVIOUS symbol).  dur_counts[b][p] is indexed by the
    phoneme of the class table, NOT by the row of `dur` (add the phonemes that share a row on the host), and has the layout of a row
    of `dur`: columns 0 .. D - 2 the expected number of runs of exactly 1 .. D - 1 frames, column D - 1 the expected number of runs of
    D frames or more, column D the expected number of frames past the D-th -- the statistics durations.reestimate takes.  An entry
    whose `trans` or `dur` is -inf is exactly 0.  logz is decode_posteriors_duration's.  A clip with status != 0 (STATUS_OVER_CAP also
    above MAX_BIGRAM_SYMBOLS; STATUS_BAD_CLASS) gets logz 0 and all-zero tables; so does an empty clip, with status 0."""
    clips = _check_clips(logits, n_frames, table, 0.0, threshold, frame_offsets)
    w = check_transitions(trans, len(clips[1]))
    d = check_duration_table(dur)
    r = check_symbol_rows(sym_dur, len(clips[1]), d.shape[0])
    D = d.shape[1] - 1
    nb, n = clips[2], len(clips[1]) + 1
    dev = logits.device
    logz = torch.empty(max(nb, 1), dtype=torch.float32, device=dev)
    succ = torch.empty((max(nb, 1), n, n), dtype=torch.float32, device=dev)
    dur_counts = torch.empty((max(nb, 1), max(n - 1, 1), D + 1), dtype=torch.float32, device=dev)
    status = torch.empty(max(nb, 1), dtype=torch.int32, device=dev)
    r_up = r if r.size else np.full(1, -1, np.int32)
    d_up = d if d.size else np.zeros((1, D + 1), np.float32)
    _call("wfl_decode_duration_counts", logits, clips, (w, r_up, d_up, int(d.shape[0]), D, float(threshold)),
          (logz, succ, dur_counts, status), stream, ws_more=(D,))
    return logz[:nb], succ[:nb], dur_counts[:nb, :n - 1], status[:nb]


def path_segments_free(ids, chunk_frames, chunk_offsets, chunk_clock, table: npost.LabelTable, frame_duration):
    """A legal path over a file's chunks (ids concatenated, chunk_frames[c] valid frames each) -> (start_s [n], end_s [n],
    phoneme index [n]) arrays, the phoneme index being table.names'.

    Each chunk goes through the native BIO decoder (no median filter) with that chunk's offsets (chunk_offsets[c]: [frames, 2] or
    None) and is shifted by its clock offset chunk_clock[c], as the free decode of Labeler.label_files.  A run that crosses a chunk
    seam (the next chunk begins with I-p of the phoneme the previous chunk ended in) is joined into one segment.  `B-p` directly after
    `B-p` or `I-p` of the same phoneme starts a new segment.  A segment's end is capped at the next segment's start, so the segments
    never overlap, and is never before its own start."""
    segs, _ = _walk_runs(ids, chunk_frames, chunk_offsets, chunk_clock, table, frame_duration)
    return (np.array([g[0] for g in segs], np.float64), np.array([g[1] for g in segs], np.float64),
            np.array([g[2] for g in segs], np.int32))


def _run_frames(idc, table: npost.LabelTable):
    """(first, end) frame of every run of one chunk's ids, as the native BIO decoder (wfl_host_decode_bio) opens and closes them: B-x
    opens a run; I-x continues an open run of x and otherwise opens one; O, the next opening and the chunk's end close it; any other
    tag is passed over."""
    rel = np.nonzero(table.kind[idc] != 3)[0]
    k, p = table.kind[idc[rel]], table.phon[idc[rel]]
    prev_k, prev_p = np.concatenate([[0], k[:-1]]), np.concatenate([[-1], p[:-1]])
    opens = (k == 1) | ((k == 2) & ((prev_k == 0) | (prev_p != p)))
    events = np.nonzero(opens | (k == 0))[0]
    at = np.nonzero(opens)[0]
    closes = np.concatenate([rel[events], [len(idc)]])           # the frame of every event, then the chunk's end
    return rel[at], closes[np.searchsorted(events, at, side="right")]


def _walk_runs(ids, chunk_frames, chunk_offsets, chunk_clock, table: npost.LabelTable, frame_duration, want_frames=False):
    """The one walk over a path's runs that path_segments_free and free_score share -> (segments [[start_s, end_s, phoneme]], frames):
    frames[j] holds the (first, end) frame ranges, in the file's concatenated frames, that make up segment j (two or more when the run
    crosses a chunk seam; only with want_frames)."""
    ids = np.asarray(ids, np.int32)
    segs, frames = [], []
    pos = 0
    last = -1                                            # the class of the previous chunk's last frame
    for Tc, offs, t0 in zip(chunk_frames, chunk_offsets, chunk_clock):
        idc = ids[pos:pos + Tc]
        base = pos
        pos += Tc
        if Tc == 0:
            continue
        s, e, ph = npost.decode_bio_ids(idc, table, frame_duration, offs, median=0)
        first = int(idc[0])
        joined = bool(len(s) and segs and last >= 0 and table.kind[first] == 2 and table.kind[last] in (1, 2)
                      and table.phon[first] == table.phon[last] and segs[-1][2] == int(ph[0]))
        if want_frames:
            starts, ends = _run_frames(idc, table)
            if len(starts) != len(s):
                raise RuntimeError(f"path decode: {len(s)} segments for {len(starts)} runs")
        for j in range(len(s)):
            f0, f1 = (int(starts[j]), int(ends[j])) if want_frames else (0, 0)
            if j == 0 and joined:                        # the run continues from the previous chunk
                segs[-1][1] = float(e[0]) + t0
                frames[-1].append((base + f0, base + f1))
            else:
                segs.append([float(s[j]) + t0, float(e[j]) + t0, int(ph[j])])
                frames.append([(base + f0, base + f1)])
        last = int(idc[-1])
    for j, g in enumerate(segs):
        if j + 1 < len(segs):                            # the decoder closes a run at the NEXT run's first frame (its end offset):
            g[1] = min(g[1], segs[j + 1][0])             # keep the segments from overlapping
        g[1] = max(g[1], g[0])
    return segs, frames


# ---------------------------------------------------------------------------------------------------------------- decode scores
class RunScore(NamedTuple):
    start_s: float              # the run's segment, as path_segments_free gives it
    end_s: float
    phoneme: str
    posterior: float            # mean over the run's frames of decode_posteriors' post: that the frame belongs to this phoneme
    start_posterior: float      # cls_post at the run's first frame: that a run of this phoneme opens exactly there
    min_frame_posterior: float  # the run's weakest frame


class FreeScore(NamedTuple):
    path_log_posterior: float        # score + sum lse - logz, <= 0: log probability of the chosen path among the legal ones
    mean_frame_logprob: float        # score / n_frames
    legal_log_mass_per_frame: float  # (logz - sum lse) / n_frames, <= 0: how much of the frames' probability the grammar keeps
    min_posterior: float             # the weakest run's posterior (1 for a path without runs)
    runs: List[RunScore]


def free_score(score, logz, sum_lse, post, cls_post, ids, chunk_frames, chunk_offsets, chunk_clock, table: npost.LabelTable,
               frame_duration, names=None):
    """One file's FreeScore from bio_viterbi's score and ids, decode_posteriors' logz / post / cls_post for the file (host values;
    per-frame arrays over the file's concatenated frames) and the sum of the frames' log-sum-exp.  The runs are walked exactly as
    path_segments_free walks them (seam joins included), so run j is segment j of the path.  names: phoneme index -> the name to
    report (default table.names)."""
    post, cls_post = np.asarray(post, np.float64).reshape(-1), np.asarray(cls_post, np.float64).reshape(-1)
    ids = np.asarray(ids, np.int32).reshape(-1)
    if not len(post) == len(cls_post) == len(ids) == int(sum(chunk_frames)):
        raise ValueError("one post, cls_post and id per frame of the chunk plan")
    segs, frames = _walk_runs(ids, chunk_frames, chunk_offsets, chunk_clock, table, frame_duration, want_frames=True)
    names = table.names if names is None else names
    runs = []
    for (s, e, ph), parts in zip(segs, frames):
        p = np.concatenate([post[a:b] for a, b in parts])
        runs.append(RunScore(float(s), float(e), str(names[ph]), float(p.mean()), float(cls_post[parts[0][0]]), float(p.min())))
    score, logz, sum_lse, n = float(score), float(logz), float(sum_lse), max(len(ids), 1)
    return FreeScore(score + sum_lse - logz, score / n, (logz - sum_lse) / n, min((r.posterior for r in runs), default=1.0), runs)
