"""BIO-grammar Viterbi decode of files WITHOUT a transcript over the model's frame logits (`postprocess.decode: viterbi`).

The reference's free decode takes each frame's argmax on its own, turns frames below `confidence_threshold` into `O`, runs a median
filter over the integer class ids and lets `decode_bio_tags` make what it can of the tag string (infer.py:86-96, 164-174, 293-302;
utils.py:47-61).  That decode knows nothing of the grammar: `I-x` straight after `B-y` or `O` silently opens a segment, a one-frame
flicker between two near-tied classes cuts a phoneme in three, and the posteriors are thrown away first.  This module instead
searches the frame logits for the best LEGAL tag string (csrc/decode.hip, include/wfl_asr.h `wfl_decode`): every `I-p` directly
follows `B-p` or `I-p`, and every run that is opened costs `switch_penalty` nats.

  class_table         label set -> (O class, (B class, I class or -1) per phoneme); every other class is never chosen
  bio_viterbi         the C ABI on CUDA tensors: a ragged batch of clips in one call
  path_segments_free  the path's ids of a file, chunk by chunk, -> segments; a run that crosses a chunk seam is one segment
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from . import native_post as npost
from ._lib import back_to_back, host_ptr as _hp, ptr as _ptr
from .align import class_pairs

DECODE_MODES = ("argmax", "viterbi")
MAX_CLASSES = 1024         # wfl_decode's class cap (status 2 above it)
STATUS_OK, STATUS_OVER_CAP, STATUS_BAD_CLASS = 0, 2, 4


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


def check_options(decode, switch_penalty):
    """Validation shared by the Labeler, infer_audio / infer_folder and the CLI (None = not given)."""
    if decode is not None and decode not in DECODE_MODES:
        raise ValueError(f"decode must be one of {DECODE_MODES}, got {decode!r}")
    if switch_penalty is not None:
        try:
            ok = float(switch_penalty) >= 0.0 and not isinstance(switch_penalty, bool)
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError(f"switch_penalty must be a number >= 0 (nats), got {switch_penalty!r}")


def workspace_bytes(n_frames, n_pairs) -> int:
    lib = _lib.load()
    T = np.ascontiguousarray(n_frames, np.int32)
    n = int(lib.wfl_decode_workspace_bytes(_hp(T), T.size, int(n_pairs)))
    if n < 0:
        raise _lib.WflError("wfl_decode_workspace_bytes: negative frame or pair count")
    return n


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
    lib = _lib.load()
    dev = logits.device
    rows = logits.shape[0]
    ws_n = workspace_bytes(T, len(pairs)) if logits.shape[1] <= MAX_CLASSES else 0
    ws = torch.empty(max(ws_n, 1), dtype=torch.uint8, device=dev)
    d_pairs = torch.from_numpy(pairs if len(pairs) else np.full((1, 2), -1, np.int32)).to(dev)
    ids = torch.empty(rows, dtype=torch.int32, device=dev)
    score = torch.empty(max(nb, 1), dtype=torch.float32, device=dev)
    status = torch.empty(max(nb, 1), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        st = stream if stream is not None else torch.cuda.current_stream(dev)
        ldl = logits.stride(0) if logits.numel() else logits.shape[1]      # (an empty tensor's strides say nothing)
        rc = lib.wfl_decode(_ptr(logits), ldl, logits.shape[1], int(o_id), _hp(F0), _hp(T), nb, _ptr(d_pairs), len(pairs),
                            float(switch_penalty), float(threshold), _ptr(ws), ws_n, _ptr(ids), _ptr(score), _ptr(status),
                            C.c_void_p(st.cuda_stream))
        _lib.check(rc, "wfl_decode")
        for t in (d_pairs, ws):
            t.record_stream(st)
    return ids, score[:nb], status[:nb]


def path_segments_free(ids, chunk_frames, chunk_offsets, chunk_clock, table: npost.LabelTable, frame_duration):
    """A legal path over a file's chunks (ids concatenated, chunk_frames[c] valid frames each) -> (start_s [n], end_s [n],
    phoneme index [n]) arrays, the phoneme index being table.names'.

    Each chunk goes through the native BIO decoder (no median filter) with that chunk's offsets (chunk_offsets[c]: [frames, 2] or
    None) and is shifted by its clock offset chunk_clock[c], as the free decode of Labeler.label_files.  A run that crosses a chunk
    seam (the next chunk begins with I-p of the phoneme the previous chunk ended in) is joined into one segment.  `B-p` directly after
    `B-p` or `I-p` of the same phoneme starts a new segment.  A segment's end is capped at the next segment's start, so the segments
    never overlap, and is never before its own start."""
    ids = np.asarray(ids, np.int32)
    segs = []                                            # [start, end, phoneme]
    pos = 0
    last = -1                                            # the class of the previous chunk's last frame
    for Tc, offs, t0 in zip(chunk_frames, chunk_offsets, chunk_clock):
        idc = ids[pos:pos + Tc]
        pos += Tc
        if Tc == 0:
            continue
        s, e, ph = npost.decode_bio_ids(idc, table, frame_duration, offs, median=0)
        first = int(idc[0])
        joined = bool(len(s) and segs and last >= 0 and table.kind[first] == 2 and table.kind[last] in (1, 2)
                      and table.phon[first] == table.phon[last] and segs[-1][2] == int(ph[0]))
        for j in range(len(s)):
            if j == 0 and joined:                        # the run continues from the previous chunk
                segs[-1][1] = float(e[0]) + t0
            else:
                segs.append([float(s[j]) + t0, float(e[j]) + t0, int(ph[j])])
        last = int(idc[-1])
    for j, g in enumerate(segs):
        if j + 1 < len(segs):                            # the decoder closes a run at the NEXT run's first frame (its end offset):
            g[1] = min(g[1], segs[j + 1][0])             # keep the segments from overlapping
        g[1] = max(g[1], g[0])
    return (np.array([g[0] for g in segs], np.float64), np.array([g[1] for g in segs], np.float64),
            np.array([g[2] for g in segs], np.int32))
