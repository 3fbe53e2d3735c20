"""Viterbi forced alignment of a transcript over the model's frame logits (`postprocess.align: viterbi`).

The reference aligns a `{audio}.txt` phoneme list by a greedy in-order string match over the freely decoded segments
(/root/reference/infer.py:30-60, applied at 312-319; restated in postprocess.align_phoneme_list).  That match never looks at the
posteriors: a missed, inserted or mislabelled phoneme shifts every later token onto the wrong segment.  This module instead searches
the frame logits for the best path that spells exactly the transcript, in order (csrc/align.hip, include/wfl_asr.h `wfl_align`): every
token gets one contiguous, time-ordered run of frames, none is dropped.

  _call                 the one call path of the entries below: workspace, argument order, stream, check (as decode._call)
  AlignBatch            a wave's ragged batch as the Labeler holds it: `windows` / `min_frames`, `select`, `pack`, `args`
  reuses_packed         whether a scoring call runs on the search's PackedClips or on tables packed again for its clips
  viterbi_align         the C ABI on CUDA tensors: a ragged batch of clips in one call; with `windows`, every token may open only
                        inside its (lo, hi) frame window (`wfl_align_windowed`, `postprocess.align_draft`); with `min_frames`,
                        every token occupies at least that many frames (`wfl_align_min_duration`, `postprocess.min_duration`)
  viterbi_align_optional  the same search where a path may leave out the tokens the caller marks (`wfl_align_optional`,
                        `postprocess.optional_tokens`), each at `skip_penalty` nats -> viterbi_align's four and `skipped` per token
  viterbi_align_filler  the same search where the tokens the caller marks are fillers: they match anything, every frame of their run
                        scoring the frame's best class minus `filler_penalty` (`wfl_align_filler`, `postprocess.filler_token`)
  filler_flags / collapse_fillers / filler_segments   `postprocess.filler_token` -> a flag per transcript token; runs of fillers merged;
                        the free segments a filler's span holds, clipped to it
  optional_flags / min_frames_needed   `postprocess.optional_tokens` -> a flag per transcript token; the frames such a transcript needs
  skipped_tokens        one file's SkippedToken rows
  optional_posteriors   forward-backward over that skip lattice (`wfl_align_optional_posterior`; `postprocess.optional_scores`):
                        alignment_posteriors' outputs and keep_post, per token the posterior probability that it is present
  optional_token_scores one file's OptionalTokenScore rows (kept | skipped, the keep posterior, the `doubt` flag)
  min_frames_for        `postprocess.min_duration` (seconds, or seconds per token name) -> frames per transcript token
  viterbi_align_duration_prior  the search with a duration prior per token: a run of d frames adds its table row's L(d)
                        (`wfl_align_duration_prior`, `postprocess.duration_prior`); upload_durations packs the rows once
  duration_rows         a durations.DurationPrior -> the table row of every transcript token (-1: none)
  duration_prior_posteriors  forward-backward over that explicit-duration lattice (`wfl_align_duration_prior_posterior`;
                        `postprocess.duration_prior_scores`): alignment_posteriors' outputs and the moments of every token's end
  filler_scores / token_durations   one file's FillerScore / TokenDuration rows from those outputs
  duration_prior_expected_counts  every token's run-length posterior over that lattice (`wfl_align_duration_prior_counts`): the
                        E-step of durations.reestimate, `python -m wfl_asr_amd.adapt_durations`
  alignment_posteriors  forward-backward over the same lattice (csrc/align_posterior.h, `wfl_align_posterior`; of a batch packed with
                        windows, `wfl_align_posterior_windowed`): logZ, and per token
                        the posterior of the run Viterbi chose and the spread of its start (`postprocess.align_scores`)
  duration_posteriors   the same over the minimum-duration lattice of a batch packed with `min_frames`
                        (`wfl_align_min_duration_posterior`; `postprocess.duration_scores`)
  edit_scores           per token the log likelihood ratio of every single substitution from a table and of the token's deletion
                        (csrc/align_edits.hip, `wfl_align_edits`; `postprocess.align_edits`), on the same lattice, windows included
  substitute_table      the (B, I) pairs of a label set, the table edit_scores takes
  edit_groups           clips -> groups whose edit_scores workspace stays under EDITS_WORKSPACE_LIMIT
  token_edits           one file's TokenEdit rows
  insertion_scores      per place (in front of every token, and behind the last) the log likelihood ratio of inserting every phoneme
                        of a table there (csrc/align_edits.hip, `wfl_align_insertions`; `postprocess.align_insertions`)
  place_insertions      one file's PlaceInsertion rows
  file_score            those outputs + viterbi_align's score -> FileScore / TokenScore records
  token_alternatives    transcript tokens -> (B, I) class pairs of every phoneme whose output name is the token
  gap_classes           the classes a gap between tokens may take (O, and SP / AP unless the transcript spells them)
  path_segments         the path's ids / tokens, chunk by chunk, -> exactly one (start, end, token) per transcript token
  windows_feasible      the host rule that predicts the windowed search's status 1
  draft_windows         a draft's start times -> per-token windows on the file's rows, through the chunk clock
  read_draft            the draft .lab of a file (phonotactics.read_lab, the HTK reader the bigram estimate uses)
  parse_variants / compile_graph   `postprocess.transcript_variants`: the `( a | b c | )` groups of a `.txt` -> its elements -> the
                        slots, predecessors and finals of a transcript graph (TranscriptGraph)
  viterbi_align_graph   the search over such graphs, choosing among the variants jointly (`wfl_align_graph`, csrc/align_graph.hip)
                        -> viterbi_align's four and `taken` per slot; chain_graph: a plain transcript as a graph; pack_graph: the
                        tables of a batch, packed and uploaded once
  variant_choices       one file's VariantChoice rows

The records of those rows (TokenEdit, PlaceInsertion, SkippedToken, OptionalTokenScore, FillerSpan, FillerScore, TokenDuration,
VariantChoice) and
the files they are written to are reports.py's; the records are imported here, so align.TokenEdit and the others name them too.
"""
from __future__ import annotations

import ctypes as C
from typing import List, NamedTuple

import numpy as np
import torch

from . import _lib
from . import native_post as npost
from ._lib import back_to_back, host_ptr as _hp, ptr as _ptr
from .reports import (FillerScore, FillerSpan, OptionalTokenScore, PlaceInsertion, SkippedToken, TokenDuration,  # noqa: F401
                      TokenEdit, VariantChoice)

MAX_TOKENS = 4096          # wfl_align's token cap per clip (status 2 above it)
MAX_ALTERNATIVES = 4       # (B, I) pairs per token
MAX_GAP = 8                # gap classes per clip
MAX_MIN_FRAMES = 8         # wfl_align_min_duration's cap on a token's minimum duration, frames (csrc/lattice.h)
MAX_PRIOR_FRAMES = 32      # wfl_align_duration_prior's cap on D, the longest explicit duration of its table (csrc/align_duration_prior.hip)
PAUSES = ("SP", "AP")

STATUS_OK, STATUS_INFEASIBLE, STATUS_OVER_CAP, STATUS_BAD_CLASS = 0, 1, 2, 4
STATUS_NOT_A_PATH = 8      # wfl_align_posterior alone: `tok` is not a path of the clip's lattice
OPEN_WINDOW = (0, 2 ** 31 - 1)   # a token that may open at any frame
MAX_SUBSTITUTES = 512      # wfl_align_edits' table cap
# edit_scores keeps about 3 N T floats per clip (5.3 MB for a 30 s clip of 300 tokens, 740 MB at the caps): the Labeler scores the
# aligned files in groups whose workspace stays under this many bytes (a single clip above it runs alone)
EDITS_WORKSPACE_LIMIT = 1 << 30


def _workspace_bytes(symbol, n_frames, n_tokens, *more) -> int:
    T = np.ascontiguousarray(n_frames, np.int32)
    N = np.ascontiguousarray(n_tokens, np.int32)
    n = int(getattr(_lib.load(), symbol)(_hp(T), _hp(N), T.size, *more))
    if n < 0:
        raise _lib.WflError(f"{symbol}: negative frame or token count" + (f", or an argument out of range {more}" if more else ""))
    return n


def workspace_bytes(n_frames, n_tokens) -> int:
    return _workspace_bytes("wfl_align_workspace_bytes", n_frames, n_tokens)


def optional_workspace_bytes(n_frames, n_tokens) -> int:
    return _workspace_bytes("wfl_align_optional_workspace_bytes", n_frames, n_tokens)


def filler_workspace_bytes(n_frames, n_tokens) -> int:
    return _workspace_bytes("wfl_align_filler_workspace_bytes", n_frames, n_tokens)


def duration_prior_workspace_bytes(n_frames, n_tokens, max_frames) -> int:
    """max_frames: D, the table's longest explicit duration (its rows have D + 1 columns), 1 .. MAX_PRIOR_FRAMES."""
    return _workspace_bytes("wfl_align_duration_prior_workspace_bytes", n_frames, n_tokens, int(max_frames))


def duration_prior_posterior_workspace_bytes(n_frames, n_tokens, max_frames) -> int:
    """max_frames: D, as duration_prior_workspace_bytes'."""
    return _workspace_bytes("wfl_align_duration_prior_posterior_workspace_bytes", n_frames, n_tokens, int(max_frames))


def duration_prior_counts_workspace_bytes(n_frames, n_tokens, max_frames) -> int:
    """max_frames: D, as duration_prior_workspace_bytes'."""
    return _workspace_bytes("wfl_align_duration_prior_counts_workspace_bytes", n_frames, n_tokens, int(max_frames))


def optional_posterior_workspace_bytes(n_frames, n_tokens) -> int:
    return _workspace_bytes("wfl_align_optional_posterior_workspace_bytes", n_frames, n_tokens)


def filler_posterior_workspace_bytes(n_frames, n_tokens) -> int:
    return _workspace_bytes("wfl_align_filler_posterior_workspace_bytes", n_frames, n_tokens)


def posterior_workspace_bytes(n_frames, n_tokens) -> int:
    return _workspace_bytes("wfl_align_posterior_workspace_bytes", n_frames, n_tokens)


def duration_posterior_workspace_bytes(n_frames, n_tokens) -> int:
    return _workspace_bytes("wfl_align_min_duration_posterior_workspace_bytes", n_frames, n_tokens)


def edits_workspace_bytes(n_frames, n_tokens) -> int:
    return _workspace_bytes("wfl_align_edits_workspace_bytes", n_frames, n_tokens)


def insertions_workspace_bytes(n_frames, n_tokens) -> int:
    return _workspace_bytes("wfl_align_insertions_workspace_bytes", n_frames, n_tokens)


def _pack_clips(logits, n_frames, token_classes, gap_classes, frame_offsets):
    """The validation and host-side packing that viterbi_align and alignment_posteriors share -> (nb, T, N, F0, K0, tc, gc)."""
    if not logits.is_cuda or logits.dim() != 2 or logits.dtype != torch.float32 or logits.stride(1) != 1:
        raise ValueError("logits must be a [rows, C] float32 CUDA tensor with contiguous rows")
    nb = len(n_frames)
    if len(token_classes) != nb or len(gap_classes) != nb:
        raise ValueError("n_frames, token_classes and gap_classes need one entry per clip")
    T = np.asarray(n_frames, np.int32).reshape(nb)
    N = np.array([len(t) for t in token_classes], np.int32)
    if frame_offsets is None:
        frame_offsets = back_to_back(T)
    F0 = np.ascontiguousarray(frame_offsets, np.int64).reshape(nb)
    K0 = np.concatenate([[0], np.cumsum(N.astype(np.int64))[:-1]]).astype(np.int32) if nb else np.zeros(0, np.int32)
    flat = [a for toks in token_classes for a in toks]
    if any(not 1 <= len(a) <= MAX_ALTERNATIVES for a in flat):
        raise ValueError(f"a token needs 1 to {MAX_ALTERNATIVES} (B, I) class pairs")
    pad = [(-1, -1)] * MAX_ALTERNATIVES
    tc = np.array([list(a) + pad[len(a):] for a in flat] or [pad], np.int32).reshape(-1, MAX_ALTERNATIVES, 2)
    gc = np.full((max(nb, 1), MAX_GAP), -1, np.int32)
    for b, g in enumerate(gap_classes):
        if not 1 <= len(g) <= MAX_GAP:
            raise ValueError(f"a clip needs 1 to {MAX_GAP} gap classes, got {len(g)}")
        gc[b, :len(g)] = g
    if nb and int((F0 + T).max()) > logits.shape[0]:
        raise ValueError("a clip's frames run past the logits rows")
    return nb, T, N, F0, K0, tc, gc


class PackedClips(NamedTuple):
    """pack_clips' result: the host arrays and the uploaded token / gap tables of a ragged batch."""
    nb: int
    T: np.ndarray
    N: np.ndarray
    F0: np.ndarray
    K0: np.ndarray
    d_tc: torch.Tensor
    d_gc: torch.Tensor
    d_win: torch.Tensor = None      # [tokens, 2] int32 (lo, hi) start windows; None: the unwindowed entries
    d_min: torch.Tensor = None      # [tokens] int32 minimum durations in frames; None: the entries without them


def _pack_windows(windows, N):
    """Per clip a list of (lo, hi) per token, or None for open windows -> [max(tokens, 1), 2] int32, rows as the token table's."""
    if len(windows) != len(N):
        raise ValueError("windows needs one entry per clip (None: open windows)")
    out = np.empty((max(int(N.sum()), 1), 2), np.int64)
    out[:] = OPEN_WINDOW
    k0 = 0
    for w, n in zip(windows, N):
        if w is not None:
            w = np.asarray(w, np.int64).reshape(-1, 2)
            if len(w) != n:
                raise ValueError(f"a clip with {n} tokens needs {n} (lo, hi) windows, got {len(w)}")
            out[k0:k0 + n] = w
        k0 += int(n)
    if out.min() < -2 ** 31 or out.max() > 2 ** 31 - 1:
        raise ValueError("window bounds are int32")
    return out.astype(np.int32)


def _pack_min_frames(min_frames, N):
    """Per clip a list of ints per token, or None for all 1 -> [max(tokens, 1)] int32, rows as the token table's.  The values are
    not judged here: a D outside 1 .. MAX_MIN_FRAMES is the kernel's STATUS_BAD_CLASS for its clip."""
    if len(min_frames) != len(N):
        raise ValueError("min_frames needs one entry per clip (None: every token 1)")
    out = np.ones(max(int(N.sum()), 1), np.int64)
    k0 = 0
    for d, n in zip(min_frames, N):
        if d is not None:
            if any(isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, np.integer)) for x in d):
                raise ValueError("min_frames are ints (frames)")
            d = np.asarray(d, np.int64).reshape(-1)
            if len(d) != n:
                raise ValueError(f"a clip with {n} tokens needs {n} minimum durations, got {len(d)}")
            out[k0:k0 + n] = d
        k0 += int(n)
    if out.min() < -2 ** 31 or out.max() > 2 ** 31 - 1:
        raise ValueError("min_frames are int32")
    return out.astype(np.int32)


def _pack_optional(optional, N):
    """Per clip a list of flags per token (bools, or ints 0 | 1), or None for a clip without optional tokens -> [max(tokens, 1)]
    int32, rows as the token table's.  The values are not judged here: a flag other than 0 | 1 is the kernel's STATUS_BAD_CLASS for
    its clip."""
    if len(optional) != len(N):
        raise ValueError("optional needs one entry per clip (None: no optional token)")
    out = np.zeros(max(int(N.sum()), 1), np.int64)
    k0 = 0
    for f, n in zip(optional, N):
        if f is not None:
            if any(not isinstance(x, (bool, np.bool_, int, np.integer)) for x in f):
                raise ValueError("optional flags are bools")
            f = np.asarray(f, np.int64).reshape(-1)
            if len(f) != n:
                raise ValueError(f"a clip with {n} tokens needs {n} optional flags, got {len(f)}")
            out[k0:k0 + n] = f
        k0 += int(n)
    if out.min() < -2 ** 31 or out.max() > 2 ** 31 - 1:
        raise ValueError("optional flags are int32")
    return out.astype(np.int32)


def _pack_fillers(fillers, N):
    """Per clip a list of flags per token (bools, or ints 0 | 1), or None for a clip without fillers -> [max(tokens, 1)] int32, rows as
    the token table's.  The values are not judged here: a flag other than 0 | 1 is the kernel's STATUS_BAD_CLASS for its clip."""
    if len(fillers) != len(N):
        raise ValueError("fillers needs one entry per clip (None: no filler)")
    out = np.zeros(max(int(N.sum()), 1), np.int64)
    k0 = 0
    for f, n in zip(fillers, N):
        if f is not None:
            if any(not isinstance(x, (bool, np.bool_, int, np.integer)) for x in f):
                raise ValueError("filler flags are bools")
            f = np.asarray(f, np.int64).reshape(-1)
            if len(f) != n:
                raise ValueError(f"a clip with {n} tokens needs {n} filler flags, got {len(f)}")
            out[k0:k0 + n] = f
        k0 += int(n)
    if out.min() < -2 ** 31 or out.max() > 2 ** 31 - 1:
        raise ValueError("filler flags are int32")
    return out.astype(np.int32)


def pack_clips(logits, n_frames, token_classes, gap_classes, frame_offsets=None, windows=None, min_frames=None) -> PackedClips:
    """Validate a ragged batch and upload its token and gap tables once; pass the result as `packed=` to viterbi_align and to
    alignment_posteriors of the same batch (the packing is host work that grows with the token count).  windows: per clip a list of
    (lo, hi) per token -- the frames, inclusive, at which the token may open -- or None for a clip with open windows; None for the
    whole batch packs for the unwindowed entries.  min_frames: per clip a list of ints per token -- the frames the token occupies at
    least, 1 .. MAX_MIN_FRAMES -- or None for a clip of all 1; None for the whole batch packs for the entries without minimum
    durations."""
    nb, T, N, F0, K0, tc, gc = _pack_clips(logits, n_frames, token_classes, gap_classes, frame_offsets)
    d_win = torch.from_numpy(_pack_windows(windows, N)).to(logits.device) if windows is not None else None
    d_min = torch.from_numpy(_pack_min_frames(min_frames, N)).to(logits.device) if min_frames is not None else None
    return PackedClips(nb, T, N, F0, K0, torch.from_numpy(tc).to(logits.device), torch.from_numpy(gc).to(logits.device), d_win, d_min)


def _any_or_none(per_clip):
    """Per-clip constraints -> the list, its Nones included, or None when no clip has any (the entries without them)."""
    return per_clip if any(x is not None for x in per_clip) else None


def reuses_packed(packed, n_clips, n_selected, with_min) -> bool:
    """Whether a scoring call over `n_selected` of a batch's `n_clips` clips runs on `packed`, the PackedClips that batch is held in
    (None: it has none), or on tables packed again for the selection.  with_min: the call is duration_posteriors, over the lattice
    with minimum durations.  The tables must hold exactly the call's clips and the call's lattice:

      packed             selected    with_min  ->
      None               any         any       pack again (the search packed for itself, or a fallback round dropped constraints)
      without durations  every clip  False     reuse      (posteriors, edits, insertions when the search aligned every clip; an edit
                                                           group that holds every aligned clip)
      without durations  some clips  False     pack again (clips left the batch with a status, or into another edit group)
      with durations     every clip  True      reuse      (every clip kept its durations)
      with durations     some clips  True      pack again
      with durations     any         False     pack again (clips that lost their durations: alignment_posteriors refuses a d_min)
      without durations  any         True      pack again (duration_posteriors refuses tables without a d_min)"""
    return packed is not None and n_selected == n_clips and (packed.d_min is not None) == bool(with_min)


class AlignBatch(NamedTuple):
    """A ragged batch as the Labeler holds it between the stages of a wave: the arguments of viterbi_align and the scoring calls,
    clip by clip.  Only pack needs the library and a GPU."""
    lg: object            # the wave's logits [rows, C]
    frames: list          # frames per clip
    f0: np.ndarray        # first row of each clip
    alts: list            # per clip its tokens' alternatives (token_alternatives)
    gaps: list            # per clip its gap classes
    wins: list            # per clip its tokens' start windows; None: none (open)
    mins: list            # per clip its tokens' minimum frames; None: none (all 1)
    o_id: int
    opts: list = None     # per clip its tokens' optional flags; None (the field or an entry): no token may be skipped
    fills: list = None    # per clip its tokens' filler flags; None (the field or an entry): no token is a filler
    durs: list = None     # per clip its tokens' rows of the duration table (-1: none); None: the searches without a duration prior

    @classmethod
    def of(cls, lg, frames, alts, gaps, o_id, wins=None, mins=None, opts=None, fills=None, durs=None):
        none = [None] * len(frames)                       # (the clips' rows one after the other in `lg`)
        return cls(lg, list(frames), back_to_back(frames), list(alts), list(gaps), list(wins or none), list(mins or none), o_id,
                   list(opts or none), list(fills) if fills is not None else None, list(durs) if durs is not None else None)

    @property
    def windows(self):
        return _any_or_none(self.wins)

    @property
    def min_frames(self):
        return _any_or_none(self.mins)

    @property
    def optional(self):
        """The per-clip flags where any clip has a flag set, else None (the entries without skip arcs)."""
        flags = self.opts or []
        return list(flags) if any(f is not None and any(f) for f in flags) else None

    @property
    def fillers(self):
        """The per-clip filler flags where any clip has a flag set, else None (the entries without a filler emission)."""
        flags = self.fills or []
        return list(flags) if any(f is not None and any(f) for f in flags) else None

    def select(self, idx):
        """The sub-batch of the clips `idx`, in that order, on the same logits."""
        idx = [int(b) for b in idx]
        fields = ("frames", "alts", "gaps", "wins", "mins") + (("opts",) if self.opts is not None else ()) \
            + (("fills",) if self.fills is not None else ()) + (("durs",) if self.durs is not None else ())
        return self._replace(f0=self.f0[idx], **{k: [getattr(self, k)[b] for b in idx] for k in fields})

    def pack(self, with_min) -> PackedClips:
        """pack_clips of the batch; with_min: the minimum durations too (a search or a score over that lattice)."""
        return pack_clips(self.lg, self.frames, self.alts, self.gaps, self.f0, windows=self.windows,
                          min_frames=self.min_frames if with_min else None)

    def args(self):                                       # the leading arguments of viterbi_align and of the scoring calls
        return self.lg, self.frames, self.alts, self.gaps, self.o_id

    def scored_on(self, idx, packed, with_min):
        """-> (select(idx), the PackedClips its scoring call runs on): `packed`, this batch's own, where reuses_packed allows."""
        sub = self.select(idx)
        return sub, packed if reuses_packed(packed, len(self.frames), len(sub.frames), with_min) else sub.pack(with_min)


def _check_tok(tok, logits):
    if not tok.is_cuda or tok.device != logits.device or tok.dtype != torch.int32 or tok.dim() != 1 or tok.stride(0) != 1 \
            or tok.shape[0] != logits.shape[0]:
        raise ValueError("tok must be viterbi_align's [rows] int32 CUDA tensor for these logits")


def _upload_substitutes(substitutes, dev):
    """edit_scores' and insertion_scores' table -> (d_sub [max(P, 1), 2] int32 on `dev`, P)."""
    sub = np.asarray(substitutes, np.int64).reshape(-1, 2)
    P = len(sub)
    if P > MAX_SUBSTITUTES:
        raise ValueError(f"at most {MAX_SUBSTITUTES} substitutes, got {P}")
    if P and (sub.min() < -2 ** 31 or sub.max() > 2 ** 31 - 1):
        raise ValueError("class ids are int32")
    return torch.from_numpy(np.ascontiguousarray(sub if P else np.zeros((1, 2)), np.int32)).to(dev), P


# entry -> (the entry whose workspace rule it shares, takes the start windows, takes the minimum durations)
_ENTRIES = {
    "wfl_align": ("wfl_align", False, False), "wfl_align_posterior": ("wfl_align_posterior", False, False),
    "wfl_align_windowed": ("wfl_align", True, False), "wfl_align_posterior_windowed": ("wfl_align_posterior", True, False),
    "wfl_align_min_duration": ("wfl_align", True, True), "wfl_align_optional": ("wfl_align_optional", True, False),
    "wfl_align_min_duration_posterior": ("wfl_align_min_duration_posterior", True, True),
    "wfl_align_edits": ("wfl_align_edits", True, False), "wfl_align_insertions": ("wfl_align_insertions", True, False),
    "wfl_align_optional_posterior": ("wfl_align_optional_posterior", True, False),
    "wfl_align_filler": ("wfl_align_filler", True, False),
    "wfl_align_filler_posterior": ("wfl_align_filler_posterior", True, False),
    "wfl_align_duration_prior": ("wfl_align_duration_prior", True, False),
    "wfl_align_duration_prior_posterior": ("wfl_align_duration_prior_posterior", True, False),
    "wfl_align_duration_prior_counts": ("wfl_align_duration_prior_counts", True, False),
    "wfl_align_graph": ("wfl_align_graph", False, False),
}


def _call(entry, logits, o_id, packed, middle, outputs, stream, temporaries=(), sized_by=()):
    """What the entries share after the packing: the workspace, the call on `stream` (default: the current one) and its check.  Every
    entry takes  logits .. token table, [windows], [minimum durations], gap table, clips, *middle, workspace, its bytes, *outputs,
    stream  (_ENTRIES; windows that were not packed go as a null pointer).  middle: a tensor goes as its pointer, anything else as
    it is; temporaries: tensors made for this call alone, kept for the stream beside the workspace and the packed tables; sized_by:
    what the entry's workspace rule takes after the clip count (wfl_align_duration_prior and its posterior: D)."""
    lib = _lib.load()
    sized_as, takes_win, takes_min = _ENTRIES[entry]
    nb, T, N, F0, K0, d_tc, d_gc, d_win, d_min = packed
    dev = logits.device
    ws_n = _workspace_bytes(sized_as + "_workspace_bytes", T, N, *sized_by)
    ws = torch.empty(max(ws_n, 1), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        st = stream if stream is not None else torch.cuda.current_stream(dev)
        args = [_ptr(logits), logits.stride(0), logits.shape[1], int(o_id), _hp(F0), _hp(T), _hp(K0), _hp(N), _ptr(d_tc)]
        args += ([_ptr(d_win)] if takes_win else []) + ([_ptr(d_min)] if takes_min else []) + [_ptr(d_gc), nb]
        args += [_ptr(m) if isinstance(m, torch.Tensor) else m for m in middle] + [_ptr(ws), ws_n] + [_ptr(t) for t in outputs]
        _lib.check(getattr(lib, entry)(*args, C.c_void_p(st.cuda_stream)), entry)
        for t in (d_tc, d_gc, ws, d_win, d_min, *temporaries):
            if t is not None:
                t.record_stream(st)


def viterbi_align(logits, n_frames, token_classes, gap_classes, o_id, frame_offsets=None, stream=None, packed=None, windows=None,
                  min_frames=None):
    """Forced alignment of a ragged batch of clips on the GPU.

    logits         [rows, C] float32 CUDA tensor (rows contiguous in C; clip b = rows frame_offsets[b] .. + n_frames[b]).  With
                   `lang_id=None` these are the language-averaged logits the forward returns, and the search runs on those.
    n_frames       frames per clip (host ints)
    token_classes  per clip, per token: 1..4 (B, I) class pairs (token_alternatives)
    gap_classes    per clip: 1..8 class ids a gap frame may take (gap_classes)
    frame_offsets  first row of each clip (default: the clips back to back)
    packed         pack_clips(...) of these same arguments, to share the packing with alignment_posteriors (default: packed here)
    windows        per clip a list of (lo, hi) per token, or None for a clip without windows: token k may open (be in B_k) only at a
                   frame lo <= t <= hi of its clip.  None (the default) runs wfl_align; anything else wfl_align_windowed, where a clip
                   whose windows no path satisfies gets STATUS_INFEASIBLE (windows_feasible predicts it).  With `packed`, the windows
                   are the ones packed there.
    min_frames     per clip a list of ints per token, or None for a clip of all 1: token k occupies at least that many frames
                   (1 .. MAX_MIN_FRAMES; min_frames_for).  None (the default) runs exactly the calls above; anything else
                   wfl_align_min_duration, with the windows if there are any: a clip whose durations (and windows) no path meets gets
                   STATUS_INFEASIBLE (windows_feasible(T, windows, min_frames) predicts it), a value outside the range
                   STATUS_BAD_CLASS.  With `packed`, the durations are the ones packed there.
    -> (ids [rows] int32, tok [rows] int32, score [clips] float32, status [clips] int32), CUDA tensors on `stream`'s device."""
    if packed is None:
        packed = pack_clips(logits, n_frames, token_classes, gap_classes, frame_offsets, windows, min_frames)
    dev, rows, nb = logits.device, logits.shape[0], packed.nb
    ids = torch.empty(rows, dtype=torch.int32, device=dev)
    tok = torch.empty(rows, dtype=torch.int32, device=dev)
    score = torch.empty(max(nb, 1), dtype=torch.float32, device=dev)
    status = torch.empty(max(nb, 1), dtype=torch.int32, device=dev)
    entry = "wfl_align_min_duration" if packed.d_min is not None else "wfl_align" if packed.d_win is None else "wfl_align_windowed"
    _call(entry, logits, o_id, packed, (), (ids, tok, score, status), stream)
    return ids, tok, score[:nb], status[:nb]


def upload_optional(optional, n_tokens, device):
    """viterbi_align_optional's flags (per clip a list of bools per token, or None) packed and uploaded once -> [max(tokens, 1)] int32
    tensor on `device`, for its `optional` argument.  n_tokens: tokens per clip (PackedClips.N)."""
    return torch.from_numpy(_pack_optional(optional, np.asarray(n_tokens, np.int32).reshape(-1))).to(device)


def viterbi_align_optional(logits, n_frames, token_classes, gap_classes, o_id, optional, skip_penalty=0.0, frame_offsets=None,
                           stream=None, packed=None, windows=None):
    """viterbi_align where a path may leave out the tokens marked optional (wfl_align_optional): at most one between two kept tokens,
    each at `skip_penalty` nats.

    optional      per clip a list of bools per token, or None for a clip without optional tokens.  The flags travel beside `packed`,
                  not in it: the same PackedClips serves viterbi_align and this call.  Or upload_optional(...) of such a list, to
                  pack and upload the flags of a batch once for several calls
    skip_penalty  nats >= 0 taken from the path's score per skipped token (0: a token is skipped wherever that is no worse)
    windows       as viterbi_align's; a skipped token's window is never consulted, so an optional token with an empty window
                  (lo > hi) is a token that must be skipped.  With `packed`, the windows are the ones packed there
    -> (ids, tok, score, status, skipped): viterbi_align's four -- a skipped token never appears in `tok`, the score is the path's
    sum minus skip_penalty per skipped token -- and skipped [tokens] int32, 1 for a token the path left out, in the order of the
    clips' tokens.  STATUS_INFEASIBLE: fewer frames than min_frames_needed(flags), or windows no path meets; STATUS_BAD_CLASS also
    for a flag other than 0 | 1.  A clip with status != 0 has skipped = 0.  With no flag set every output is viterbi_align's."""
    if packed is None:
        packed = pack_clips(logits, n_frames, token_classes, gap_classes, frame_offsets, windows)
    if packed.d_min is not None:
        raise ValueError("viterbi_align_optional has no minimum durations: this batch was packed with min_frames")
    lam = float(skip_penalty)
    if not (0.0 <= lam < float("inf")):
        raise ValueError("skip_penalty must be a number of nats >= 0")
    dev, rows, nb, ntok = logits.device, logits.shape[0], packed.nb, int(packed.N.sum())
    d_opt = optional if isinstance(optional, torch.Tensor) else upload_optional(optional, packed.N, dev)
    if d_opt.device != dev or d_opt.dtype != torch.int32 or d_opt.dim() != 1 or d_opt.stride(0) != 1 or d_opt.shape[0] != max(ntok, 1):
        raise ValueError("uploaded optional flags must be upload_optional's [tokens] int32 tensor for this batch")
    ids = torch.empty(rows, dtype=torch.int32, device=dev)
    tok = torch.empty(rows, dtype=torch.int32, device=dev)
    score = torch.empty(max(nb, 1), dtype=torch.float32, device=dev)
    status = torch.empty(max(nb, 1), dtype=torch.int32, device=dev)
    skipped = torch.empty(max(ntok, 1), dtype=torch.int32, device=dev)
    _call("wfl_align_optional", logits, o_id, packed, (d_opt, lam), (ids, tok, score, skipped, status), stream, temporaries=(d_opt,))
    return ids, tok, score[:nb], status[:nb], skipped[:ntok]


def _pack_durations(tok_rows, N):
    """Per clip a list of table rows per token (ints; -1: the token has no prior), or None for a clip without any -> [max(tokens, 1)]
    int32, rows as the token table's.  The values are not judged here: a row outside -1 .. n_rows - 1 is the kernel's
    STATUS_BAD_CLASS for its clip."""
    if len(tok_rows) != len(N):
        raise ValueError("tok_rows needs one entry per clip (None: no token has a prior)")
    out = np.full(max(int(N.sum()), 1), -1, np.int64)
    k0 = 0
    for d, n in zip(tok_rows, N):
        if d is not None:
            if any(isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, np.integer)) for x in d):
                raise ValueError("tok_rows are ints (rows of the duration table, -1 for none)")
            d = np.asarray(d, np.int64).reshape(-1)
            if len(d) != n:
                raise ValueError(f"a clip with {n} tokens needs {n} table rows, got {len(d)}")
            out[k0:k0 + n] = d
        k0 += int(n)
    if out.min() < -2 ** 31 or out.max() > 2 ** 31 - 1:
        raise ValueError("tok_rows are int32")
    return out.astype(np.int32)


def upload_durations(tok_rows, n_tokens, device):
    """viterbi_align_duration_prior's rows (per clip a list of ints per token, or None) packed and uploaded once -> [max(tokens, 1)]
    int32 tensor on `device`, for its `tok_rows` argument.  n_tokens: tokens per clip (PackedClips.N)."""
    return torch.from_numpy(_pack_durations(tok_rows, np.asarray(n_tokens, np.int32).reshape(-1))).to(device)


def duration_rows(transcript, prior):
    """The duration table's row of every transcript token (`postprocess.duration_prior`) -> [int] for viterbi_align_duration_prior's
    tok_rows.  prior: durations.DurationPrior; names are the transcript's own tokens, i.e. output names, as min_frames_for's.  A token
    the prior does not hold, or holds without any sample (`log_prob` null), gets -1: no prior."""
    row = {name: i for i, name in enumerate(prior.phonemes) if prior.log_prob[i] is not None}
    return [row.get(t, -1) for t in transcript]


def viterbi_align_duration_prior(logits, n_frames, token_classes, gap_classes, o_id, tok_rows, table, frame_offsets=None, stream=None,
                                 packed=None, windows=None):
    """viterbi_align with a duration prior: an explicit-duration search in which a run of d frames of a token adds its row's L(d) to
    the path's score (wfl_align_duration_prior).

    tok_rows  per clip a list of ints per token -- the token's row of `table`, -1 for a token without prior -- or None for a clip
              without any; or upload_durations(...) of such a list.  The rows travel beside `packed`, not in it
    table     [rows, D + 1] float32 (numpy, or a CUDA tensor already on the device; durations.table): columns 0 .. D - 1 are
              L(1) .. L(D), column D the tail, added once per frame past D.  Entries are finite or -inf (-inf forbids the duration),
              never NaN or +inf; the tail is <= 0 or -inf.  1 <= D <= MAX_PRIOR_FRAMES
    windows   as viterbi_align's.  With `packed`, the ones packed there.  A batch packed with `min_frames` is refused
    -> (ids, tok, score, status): viterbi_align's four; the score is the path's sum of log posteriors plus its runs' L.
    STATUS_INFEASIBLE: fewer frames than tokens, or the table (and the windows) forbid every path; STATUS_BAD_CLASS also for a row
    outside -1 .. rows - 1."""
    if packed is None:
        packed = pack_clips(logits, n_frames, token_classes, gap_classes, frame_offsets, windows)
    if packed.d_min is not None:
        raise ValueError("viterbi_align_duration_prior has no minimum durations: this batch was packed with min_frames")
    dev, rows, nb, ntok = logits.device, logits.shape[0], packed.nb, int(packed.N.sum())
    d_tab, n_rows, D = _upload_duration_table(table, dev)
    d_dur = tok_rows if isinstance(tok_rows, torch.Tensor) else upload_durations(tok_rows, packed.N, dev)
    if d_dur.device != dev or d_dur.dtype != torch.int32 or d_dur.dim() != 1 or d_dur.stride(0) != 1 or d_dur.shape[0] != max(ntok, 1):
        raise ValueError("uploaded table rows must be upload_durations' [tokens] int32 tensor for this batch")
    ids = torch.empty(rows, dtype=torch.int32, device=dev)
    tok = torch.empty(rows, dtype=torch.int32, device=dev)
    score = torch.empty(max(nb, 1), dtype=torch.float32, device=dev)
    status = torch.empty(max(nb, 1), dtype=torch.int32, device=dev)
    _call("wfl_align_duration_prior", logits, o_id, packed, (d_dur, d_tab, n_rows, D), (ids, tok, score, status), stream,
          temporaries=(d_dur, d_tab), sized_by=(D,))
    return ids, tok, score[:nb], status[:nb]


def _upload_duration_table(table, dev):
    """viterbi_align_duration_prior's and duration_prior_posteriors' `table` -> (d_tab on `dev`, n_rows, D)."""
    if isinstance(table, torch.Tensor):
        d_tab = table
        if d_tab.device != dev or d_tab.dtype != torch.float32 or d_tab.dim() != 2 or not d_tab.is_contiguous():
            raise ValueError("an uploaded duration table must be a contiguous [rows, D + 1] float32 tensor on the logits' device")
    else:
        tab = np.ascontiguousarray(table, np.float32)
        if tab.ndim != 2:
            raise ValueError("the duration table is [rows, D + 1]")
        if np.isnan(tab).any() or np.isposinf(tab).any():
            raise ValueError("duration table entries are finite or -inf")
        d_tab = torch.from_numpy(tab if tab.size else np.zeros((1, max(tab.shape[1], 2)), np.float32)).to(dev)
    n_rows, D = int(table.shape[0]), int(table.shape[1]) - 1
    if not 1 <= D <= MAX_PRIOR_FRAMES:
        raise ValueError(f"the duration table needs 2 to {MAX_PRIOR_FRAMES + 1} columns (D + 1), got {D + 1}")
    return d_tab, n_rows, D


def duration_prior_posteriors(logits, n_frames, token_classes, gap_classes, o_id, tok_rows, table, tok, frame_offsets=None, stream=None,
                              packed=None, windows=None):
    """alignment_posteriors over the explicit-duration lattice of viterbi_align_duration_prior, for the same ragged batch of clips (same
    arguments, the same `tok_rows` and `table`), given its `tok` (wfl_align_duration_prior_posterior).  A path weighs
    exp(sum of its frames' log posteriors + sum of its runs' L(d)).

    tok_rows, table  as viterbi_align_duration_prior's
    windows          as viterbi_align_duration_prior's; with `packed` -- the PackedClips the search ran on -- the ones packed there.  A
                     batch packed with `min_frames` is refused
    -> (logz, tok_post, start_mean, start_sd, end_mean, end_sd, status): per clip logz [clips] float32 and status [clips] int32; per
    token, in the order of the clips' tokens, tok_post (the posterior that the frames the search gave the token belong to it, their
    mean, in [0, 1]), start_mean / start_sd and end_mean / end_sd (mean relative to the first / last frame the search gave the token,
    and standard deviation, of the frame its run opens / ends on, in frames).  STATUS_INFEASIBLE: fewer frames than tokens, or the
    table (and the windows) leave no path; STATUS_BAD_CLASS also for a row outside -1 .. rows - 1; STATUS_NOT_A_PATH: `tok` is not a
    path of this lattice (a run of a length the table forbids included).  A clip with status != 0 gets zeros.  Large batches run in
    groups whose workspace stays under EDITS_WORKSPACE_LIMIT (edit_groups), each clip's outputs the same as in one call."""
    if packed is None:
        packed = pack_clips(logits, n_frames, token_classes, gap_classes, frame_offsets, windows)
    if packed.d_min is not None:
        raise ValueError("duration_prior_posteriors has no minimum durations: this batch was packed with min_frames")
    _check_tok(tok, logits)
    nb, ntok, dev = packed.nb, int(packed.N.sum()), logits.device
    d_tab, n_rows, D = _upload_duration_table(table, dev)
    d_dur = tok_rows if isinstance(tok_rows, torch.Tensor) else upload_durations(tok_rows, packed.N, dev)
    if d_dur.device != dev or d_dur.dtype != torch.int32 or d_dur.dim() != 1 or d_dur.stride(0) != 1 or d_dur.shape[0] != max(ntok, 1):
        raise ValueError("uploaded table rows must be upload_durations' [tokens] int32 tensor for this batch")
    logz = torch.empty(max(nb, 1), dtype=torch.float32, device=dev)
    per_tok = torch.empty((5, max(ntok, 1)), dtype=torch.float32, device=dev)
    status = torch.empty(max(nb, 1), dtype=torch.int32, device=dev)
    groups = edit_groups(packed.T, packed.N, workspace_bytes=lambda t, n: duration_prior_posterior_workspace_bytes(t, n, D))
    for grp in groups or [[]]:
        # a group is a run of consecutive clips: the host arrays are sliced, the device tables and the outputs stay whole (the token
        # offsets K0 and the clip index of gap_classes / logz / status are rebased by pointer arithmetic on the tensors' views)
        if len(groups) <= 1:
            sub, lo = packed, 0
        else:
            lo, hi = grp[0], grp[-1] + 1
            sub = packed._replace(nb=hi - lo, T=packed.T[lo:hi], N=packed.N[lo:hi], F0=packed.F0[lo:hi], K0=packed.K0[lo:hi],
                                  d_gc=packed.d_gc[lo:hi])
        _call("wfl_align_duration_prior_posterior", logits, o_id, sub, (d_dur, d_tab, n_rows, D, tok),
              (logz[lo:], per_tok[0], per_tok[1], per_tok[2], per_tok[3], per_tok[4], status[lo:]), stream,
              temporaries=(d_dur, d_tab), sized_by=(D,))
    return (logz[:nb], per_tok[0, :ntok], per_tok[1, :ntok], per_tok[2, :ntok], per_tok[3, :ntok], per_tok[4, :ntok], status[:nb])


def duration_prior_expected_counts(logits, n_frames, token_classes, gap_classes, o_id, tok_rows, table, frame_offsets=None, stream=None,
                                   packed=None, windows=None):
    """The posterior distribution of every token's run length over the explicit-duration lattice of viterbi_align_duration_prior, for
    the same ragged batch of clips (same arguments, the same `tok_rows` and `table`; no `tok`: the sums run over all paths) -- the
    E-step of durations.reestimate (wfl_align_duration_prior_counts).

    tok_rows, table  as viterbi_align_duration_prior's
    windows          as viterbi_align_duration_prior's; with `packed`, the ones packed there.  A batch packed with `min_frames` is
                     refused
    -> (logz [clips] float32, dur_post [tokens, D + 1] float32, status [clips] int32): a token's row, in the order of the clips'
    tokens, has the layout of a table row -- columns 0 .. D - 2 are P(d = 1) .. P(d = D - 1), column D - 1 is P(d >= D), column D is
    E[max(d - D, 0)]: what durations.estimate counts in `.lab` files.  An entry the table forbids is exactly 0.  A token whose row is
    -1 is computed like any other, with L = 0 and tail 0.  STATUS_INFEASIBLE: fewer frames than tokens, or the table (and the windows)
    leave no path; STATUS_BAD_CLASS also for a row outside -1 .. rows - 1.  A clip with status != 0 gets zeros.  Large batches run in
    groups whose workspace stays under EDITS_WORKSPACE_LIMIT (edit_groups), each clip's outputs the same as in one call."""
    if packed is None:
        packed = pack_clips(logits, n_frames, token_classes, gap_classes, frame_offsets, windows)
    if packed.d_min is not None:
        raise ValueError("duration_prior_expected_counts has no minimum durations: this batch was packed with min_frames")
    nb, ntok, dev = packed.nb, int(packed.N.sum()), logits.device
    d_tab, n_rows, D = _upload_duration_table(table, dev)
    d_dur = tok_rows if isinstance(tok_rows, torch.Tensor) else upload_durations(tok_rows, packed.N, dev)
    if d_dur.device != dev or d_dur.dtype != torch.int32 or d_dur.dim() != 1 or d_dur.stride(0) != 1 or d_dur.shape[0] != max(ntok, 1):
        raise ValueError("uploaded table rows must be upload_durations' [tokens] int32 tensor for this batch")
    logz = torch.empty(max(nb, 1), dtype=torch.float32, device=dev)
    dur_post = torch.empty((max(ntok, 1), D + 1), dtype=torch.float32, device=dev)
    status = torch.empty(max(nb, 1), dtype=torch.int32, device=dev)
    groups = edit_groups(packed.T, packed.N, workspace_bytes=lambda t, n: duration_prior_counts_workspace_bytes(t, n, D))
    for grp in groups or [[]]:
        if len(groups) <= 1:                 # (groups of consecutive clips, as duration_prior_posteriors')
            sub, lo = packed, 0
        else:
            lo, hi = grp[0], grp[-1] + 1
            sub = packed._replace(nb=hi - lo, T=packed.T[lo:hi], N=packed.N[lo:hi], F0=packed.F0[lo:hi], K0=packed.K0[lo:hi],
                                  d_gc=packed.d_gc[lo:hi])
        _call("wfl_align_duration_prior_counts", logits, o_id, sub, (d_dur, d_tab, n_rows, D), (logz[lo:], dur_post, status[lo:]),
              stream, temporaries=(d_dur, d_tab), sized_by=(D,))
    return logz[:nb], dur_post[:ntok], status[:nb]


def upload_filler(fillers, n_tokens, device):
    """viterbi_align_filler's flags (per clip a list of bools per token, or None) packed and uploaded once -> [max(tokens, 1)] int32
    tensor on `device`, for its `fillers` argument.  n_tokens: tokens per clip (PackedClips.N)."""
    return torch.from_numpy(_pack_fillers(fillers, np.asarray(n_tokens, np.int32).reshape(-1))).to(device)


def viterbi_align_filler(logits, n_frames, token_classes, gap_classes, o_id, fillers, filler_penalty=1.0, frame_offsets=None,
                         stream=None, packed=None, windows=None):
    """viterbi_align where the tokens marked as fillers match anything (wfl_align_filler): a filler is a token like any other -- one
    contiguous run of at least one frame, in order, gaps possible on both sides -- and in every frame of its run it scores the frame's
    largest logit over all classes minus `filler_penalty`.

    fillers         per clip a list of bools per token, or None for a clip without fillers.  The flags travel beside `packed`, not in
                    it: the same PackedClips serves viterbi_align and this call.  Or upload_filler(...) of such a list.  A filler's
                    entry of token_classes is a placeholder, one valid pair ((o_id, o_id); token_alternatives writes it): never read
    filler_penalty  nats >= 0 per frame: a frame goes to a filler instead of a neighbouring token only where that token's class is
                    more than this below the frame's best class (1.0 is a value to start from, not a measured optimum)
    windows         as viterbi_align's; a filler's window masks its opening like any token's.  With `packed`, the ones packed there.
                    A batch packed with `min_frames` is refused
    -> (ids, tok, score, status): viterbi_align's four.  In a filler's frames tok is the filler's index and ids the frame's first
    arg-max class over all classes.  STATUS_BAD_CLASS also for a flag other than 0 | 1.  With no flag set every output is
    viterbi_align's."""
    if packed is None:
        packed = pack_clips(logits, n_frames, token_classes, gap_classes, frame_offsets, windows)
    if packed.d_min is not None:
        raise ValueError("viterbi_align_filler has no minimum durations: this batch was packed with min_frames")
    phi = float(filler_penalty)
    if not (0.0 <= phi < float("inf")):
        raise ValueError("filler_penalty must be a number of nats >= 0")
    dev, rows, nb, ntok = logits.device, logits.shape[0], packed.nb, int(packed.N.sum())
    d_fill = fillers if isinstance(fillers, torch.Tensor) else upload_filler(fillers, packed.N, dev)
    if d_fill.device != dev or d_fill.dtype != torch.int32 or d_fill.dim() != 1 or d_fill.stride(0) != 1 or d_fill.shape[0] != max(ntok, 1):
        raise ValueError("uploaded filler flags must be upload_filler's [tokens] int32 tensor for this batch")
    ids = torch.empty(rows, dtype=torch.int32, device=dev)
    tok = torch.empty(rows, dtype=torch.int32, device=dev)
    score = torch.empty(max(nb, 1), dtype=torch.float32, device=dev)
    status = torch.empty(max(nb, 1), dtype=torch.int32, device=dev)
    _call("wfl_align_filler", logits, o_id, packed, (d_fill, phi), (ids, tok, score, status), stream, temporaries=(d_fill,))
    return ids, tok, score[:nb], status[:nb]


def filler_posteriors(logits, n_frames, token_classes, gap_classes, o_id, fillers, tok, filler_penalty=1.0, frame_offsets=None,
                      stream=None, packed=None, windows=None):
    """alignment_posteriors over the filler lattice of viterbi_align_filler, for the same ragged batch of clips (same arguments, the
    same `fillers` and `filler_penalty`), given its `tok` (wfl_align_filler_posterior).  A flagged token emits, in every frame, the
    frame's largest log-probability over all classes minus `filler_penalty`; everything else is alignment_posteriors' lattice.

    fillers  as viterbi_align_filler's: per clip a list of bools per token (or None), or upload_filler's tensor
    windows  as viterbi_align_filler's; with `packed` -- the PackedClips the search ran on -- the ones packed there.  A batch packed
             with `min_frames` is refused
    -> (logz, tok_post, start_mean, start_sd, end_mean, end_sd, status): alignment_posteriors' tensors and, per token, end_mean /
    end_sd [tokens] float32: mean (relative to the last frame Viterbi gave the token) and standard deviation of the frame the
    token's run ends on, in frames.  For a filler tok_post is the posterior that the frames of its span belong to the filler.
    STATUS_BAD_CLASS also for a flag other than 0 | 1; a clip with status != 0 gets zeros."""
    if packed is None:
        packed = pack_clips(logits, n_frames, token_classes, gap_classes, frame_offsets, windows)
    if packed.d_min is not None:
        raise ValueError("filler_posteriors has no minimum durations: this batch was packed with min_frames")
    phi = float(filler_penalty)
    if not (0.0 <= phi < float("inf")):
        raise ValueError("filler_penalty must be a number of nats >= 0")
    _check_tok(tok, logits)
    nb, ntok, dev = packed.nb, int(packed.N.sum()), logits.device
    d_fill = fillers if isinstance(fillers, torch.Tensor) else upload_filler(fillers, packed.N, dev)
    if d_fill.device != dev or d_fill.dtype != torch.int32 or d_fill.dim() != 1 or d_fill.stride(0) != 1 or d_fill.shape[0] != max(ntok, 1):
        raise ValueError("uploaded filler flags must be upload_filler's [tokens] int32 tensor for this batch")
    logz = torch.empty(max(nb, 1), dtype=torch.float32, device=dev)
    per_tok = torch.empty((5, max(ntok, 1)), dtype=torch.float32, device=dev)
    status = torch.empty(max(nb, 1), dtype=torch.int32, device=dev)
    _call("wfl_align_filler_posterior", logits, o_id, packed, (d_fill, phi, tok),
          (logz, per_tok[0], per_tok[1], per_tok[2], per_tok[3], per_tok[4], status), stream, temporaries=(d_fill,))
    return (logz[:nb], per_tok[0, :ntok], per_tok[1, :ntok], per_tok[2, :ntok], per_tok[3, :ntok], per_tok[4, :ntok], status[:nb])


def _optional_call_args(optional, skip_penalty, packed, logits, what):
    """The flags and the penalty as viterbi_align_optional judges them -> (d_opt, lam)."""
    if packed.d_min is not None:
        raise ValueError(f"{what} has no minimum durations: this batch was packed with min_frames")
    lam = float(skip_penalty)
    if not (0.0 <= lam < float("inf")):
        raise ValueError("skip_penalty must be a number of nats >= 0")
    ntok, dev = int(packed.N.sum()), logits.device
    d_opt = optional if isinstance(optional, torch.Tensor) else upload_optional(optional, packed.N, dev)
    if d_opt.device != dev or d_opt.dtype != torch.int32 or d_opt.dim() != 1 or d_opt.stride(0) != 1 or d_opt.shape[0] != max(ntok, 1):
        raise ValueError("uploaded optional flags must be upload_optional's [tokens] int32 tensor for this batch")
    return d_opt, lam


def optional_posteriors(logits, n_frames, token_classes, gap_classes, o_id, optional, tok, skip_penalty=0.0, frame_offsets=None,
                        stream=None, packed=None, windows=None):
    """alignment_posteriors over the skip lattice of viterbi_align_optional, for the same ragged batch of clips (same arguments,
    the same `optional` and `skip_penalty`), given its `tok` (wfl_align_optional_posterior).  A path weighs
    exp(sum of its emissions - skip_penalty per skipped token).

    optional  as viterbi_align_optional's: per clip a list of bools per token (or None), or upload_optional's tensor
    windows   as viterbi_align_optional's; with `packed` -- the PackedClips the search ran on -- the ones packed there.  A batch
              packed with `min_frames` is refused
    -> (logz, keep_post, tok_post, start_mean, start_sd, status): alignment_posteriors' tensors and keep_post [tokens] float32, the
    sum over the frames of gamma(B_k).  Every labelling is exactly one path of this lattice and a path enters B_k at most once, so
    keep_post is the posterior probability that the token is present (1 for a token that is not optional and has no optional
    neighbour to be traded against).  tok_post is 0 for a token `tok` does not hold; start_mean / start_sd are conditional on the
    token being kept, relative to Viterbi's start for a token in `tok` and to the clip's frame 0 for a skipped one.
    STATUS_NOT_A_PATH: `tok` misses a token that is not optional, or two neighbours, or opens a token outside its window."""
    if packed is None:
        packed = pack_clips(logits, n_frames, token_classes, gap_classes, frame_offsets, windows)
    d_opt, lam = _optional_call_args(optional, skip_penalty, packed, logits, "optional_posteriors")
    _check_tok(tok, logits)
    nb, ntok, dev = packed.nb, int(packed.N.sum()), logits.device
    logz = torch.empty(max(nb, 1), dtype=torch.float32, device=dev)
    per_tok = torch.empty((4, max(ntok, 1)), dtype=torch.float32, device=dev)
    status = torch.empty(max(nb, 1), dtype=torch.int32, device=dev)
    _call("wfl_align_optional_posterior", logits, o_id, packed, (d_opt, lam, tok),
          (logz, per_tok[0], per_tok[1], per_tok[2], per_tok[3], status), stream, temporaries=(d_opt,))
    return logz[:nb], per_tok[0, :ntok], per_tok[1, :ntok], per_tok[2, :ntok], per_tok[3, :ntok], status[:nb]


def _without_min_frames(packed, what):
    """The sums of alignment_posteriors, edit_scores and insertion_scores run over the lattice WITHOUT minimum durations: a batch
    packed with them is refused, a score must speak of the lattice its search ran on."""
    if packed.d_min is not None:
        raise ValueError(f"{what} scores the lattice without minimum durations: this batch was packed with min_frames")
    return packed[:8]


def _with_min_frames(packed, what):
    """The sums of duration_posteriors run over the lattice WITH minimum durations: a batch packed without them is refused, a score
    must speak of the lattice its search ran on."""
    if packed.d_min is None:
        raise ValueError(f"{what} scores the lattice with minimum durations: this batch was packed without min_frames")
    return packed


def _posteriors(entry, logits, o_id, tok, packed, stream):
    """The forward-backward entries' outputs and call -> alignment_posteriors' five tensors."""
    _check_tok(tok, logits)
    nb, ntok, dev = packed.nb, int(packed.N.sum()), logits.device
    logz = torch.empty(max(nb, 1), dtype=torch.float32, device=dev)
    per_tok = torch.empty((3, max(ntok, 1)), dtype=torch.float32, device=dev)
    status = torch.empty(max(nb, 1), dtype=torch.int32, device=dev)
    _call(entry, logits, o_id, packed, (tok,), (logz, per_tok[0], per_tok[1], per_tok[2], status), stream)
    return logz[:nb], per_tok[0, :ntok], per_tok[1, :ntok], per_tok[2, :ntok], status[:nb]


def alignment_posteriors(logits, n_frames, token_classes, gap_classes, o_id, tok, frame_offsets=None, stream=None, packed=None):
    """Forward-backward over the lattice of viterbi_align, for the same ragged batch of clips (same arguments), given its `tok`.

    tok     [rows] int32 CUDA tensor: viterbi_align's output for these clips (row frame_offsets[b] + t)
    packed  the pack_clips(...) result that viterbi_align ran on, when the batch is the same (default: packed here).  Start windows
            reach this function only through it: a batch packed with `windows` is scored by wfl_align_posterior_windowed, the sums
            running over the windowed lattice (a `tok` with a token that opens outside its window is STATUS_NOT_A_PATH), so a
            search and its scores share one lattice by sharing one PackedClips
    -> (logz [clips], tok_post [tokens], start_mean [tokens], start_sd [tokens], status [clips]): float32 / int32 CUDA tensors, the
    per-token ones in the order of the clips' tokens.  logz: log of the summed weight of every path that spells the transcript;
    tok_post: the posterior occupancy of the run Viterbi gave the token, in [0, 1]; start_mean / start_sd: mean (relative to
    Viterbi's start) and standard deviation of the token's start, in frames.  A clip with status != 0 gets zeros
    (STATUS_NOT_A_PATH: `tok` does not hold every token of the clip)."""
    if packed is None:
        packed = pack_clips(logits, n_frames, token_classes, gap_classes, frame_offsets)
    _without_min_frames(packed, "alignment_posteriors")
    entry = "wfl_align_posterior" if packed.d_win is None else "wfl_align_posterior_windowed"
    return _posteriors(entry, logits, o_id, tok, packed, stream)


def duration_posteriors(logits, n_frames, token_classes, gap_classes, o_id, tok, frame_offsets=None, stream=None, packed=None,
                        windows=None, min_frames=None):
    """alignment_posteriors over the minimum-duration lattice of viterbi_align(..., min_frames=...), for the same ragged batch of
    clips (same arguments), given its `tok` (wfl_align_min_duration_posterior).

    windows, min_frames  as viterbi_align's.  With `packed` -- the PackedClips the search ran on -- the windows and durations are
                         the ones packed there.  A batch without durations (min_frames None, or packed without them) is refused:
                         alignment_posteriors scores that lattice
    -> alignment_posteriors' five tensors.  logz: log of the summed weight of every path that gives every token its minimum
    duration (and opens it inside its window); tok_post: the posterior of being in any state of the token -- B_k, its chain, I_k --
    averaged over the run Viterbi gave it; start_mean / start_sd from B_k as there.  STATUS_NOT_A_PATH also for a `tok` with a run
    shorter than its minimum, STATUS_INFEASIBLE also when no path meets the durations, STATUS_BAD_CLASS also for a duration outside
    1 .. MAX_MIN_FRAMES."""
    if packed is None:
        packed = pack_clips(logits, n_frames, token_classes, gap_classes, frame_offsets, windows, min_frames)
    _with_min_frames(packed, "duration_posteriors")
    return _posteriors("wfl_align_min_duration_posterior", logits, o_id, tok, packed, stream)


def edit_scores(logits, n_frames, token_classes, gap_classes, o_id, substitutes, frame_offsets=None, stream=None, packed=None):
    """Single-edit scores of the transcripts of a ragged batch of clips (viterbi_align's arguments), on the lattice of the search.

    substitutes  P (B class, I class) pairs, 0 <= P <= MAX_SUBSTITUTES (substitute_table)
    packed       the pack_clips(...) result the search ran on; start windows reach this function only through it, as they reach
                 alignment_posteriors: a batch packed with `windows` is scored on the windowed lattice
    -> (logz [clips] float32, edits [tokens, P + 1] float32, status [clips] int32), CUDA tensors, the rows in the order of the clips'
    tokens.  edits[k, p] = logZ(transcript with token k replaced by substitute p alone) - logZ(transcript), edits[k, P] the same for
    the transcript without token k (and without its window): positive where the edit explains the audio better, -inf where the
    edited transcript has no path.  logz is alignment_posteriors' logz.  A clip with status != 0 gets zeros; a class id of
    `substitutes` outside the logits' columns is STATUS_BAD_CLASS for every clip."""
    if packed is None:
        packed = pack_clips(logits, n_frames, token_classes, gap_classes, frame_offsets)
    _without_min_frames(packed, "edit_scores")
    dev, nb, ntok = logits.device, packed.nb, int(packed.N.sum())
    d_sub, P = _upload_substitutes(substitutes, dev)
    logz = torch.empty(max(nb, 1), dtype=torch.float32, device=dev)
    edits = torch.empty((max(ntok, 1), P + 1), dtype=torch.float32, device=dev)
    status = torch.empty(max(nb, 1), dtype=torch.int32, device=dev)
    _call("wfl_align_edits", logits, o_id, packed, (d_sub, P), (logz, edits, status), stream, temporaries=(d_sub,))
    return logz[:nb], edits[:ntok], status[:nb]


def insertion_scores(logits, n_frames, token_classes, gap_classes, o_id, substitutes, frame_offsets=None, stream=None, packed=None):
    """Single-insertion scores of the transcripts of a ragged batch of clips (edit_scores' arguments), on the lattice of the search.

    substitutes  P (B class, I class) pairs, 0 <= P <= MAX_SUBSTITUTES (substitute_table)
    packed       the pack_clips(...) result the search ran on; start windows reach this function only through it, as they reach
                 edit_scores.  The inserted token has no window; every other token keeps its own
    -> (logz [clips] float32, ins [tokens + clips, P] float32, status [clips] int32), CUDA tensors.  A clip of N tokens has N + 1
    places -- place j in front of token j, place N behind the last token -- and owns the rows (its first token's row + its index in
    the batch) + j.  ins[row, p] = logZ(transcript with substitute p inserted at the place) - logZ(transcript): positive where the
    longer transcript explains the audio better, -inf where it has no path (every entry of a clip with as many tokens as frames).
    logz is alignment_posteriors' logz.  A clip with status != 0 gets zeros; a class id of `substitutes` outside the logits' columns
    is STATUS_BAD_CLASS for every clip."""
    if packed is None:
        packed = pack_clips(logits, n_frames, token_classes, gap_classes, frame_offsets)
    _without_min_frames(packed, "insertion_scores")
    dev, nb, rows = logits.device, packed.nb, int(packed.N.sum()) + packed.nb
    d_sub, P = _upload_substitutes(substitutes, dev)
    logz = torch.empty(max(nb, 1), dtype=torch.float32, device=dev)
    ins = torch.empty((max(rows, 1), max(P, 1)), dtype=torch.float32, device=dev)
    status = torch.empty(max(nb, 1), dtype=torch.int32, device=dev)
    _call("wfl_align_insertions", logits, o_id, packed, (d_sub, P), (logz, ins, status), stream, temporaries=(d_sub,))
    return logz[:nb], ins[:rows, :P], status[:nb]



def substitute_table(label_list):
    """-> (names, pairs): every phoneme of the label set that has both tags, in label order (of its B- tag), and its (B class,
    I class) pair -- the table edit_scores takes."""
    pairs = class_pairs(label_list)
    names = [tag[2:] for tag in label_list if tag.startswith("B-") and tag[2:] in pairs]
    return names, [pairs[ph] for ph in names]


def edit_groups(n_frames, n_tokens, limit=None, workspace_bytes=edits_workspace_bytes):
    """Indices of the clips, in order, in groups whose edit_scores workspace stays under `limit` bytes (EDITS_WORKSPACE_LIMIT); a
    clip that is over it alone is a group of its own.  workspace_bytes: the scoring call's own rule (insertions_workspace_bytes for
    insertion_scores)."""
    limit = EDITS_WORKSPACE_LIMIT if limit is None else limit
    groups, cur, used = [], [], 0
    for j, (t, n) in enumerate(zip(n_frames, n_tokens)):
        need = workspace_bytes([t], [n])
        if cur and used + need > limit:
            groups.append(cur)
            cur, used = [], 0
        cur.append(j)
        used += need
    if cur:
        groups.append(cur)
    return groups


# ---------------------------------------------------------------------------------------------------------------- host helpers
def class_pairs(label_list):
    """phoneme name (as in the label set) -> (B class, I class), for the phonemes that have both tags."""
    b, i = {}, {}
    for c, tag in enumerate(label_list):
        if tag.startswith("B-"):
            b[tag[2:]] = c
        elif tag.startswith("I-"):
            i[tag[2:]] = c
    return {ph: (b[ph], i[ph]) for ph in b if ph in i}


def token_alternatives(transcript, table: npost.LabelTable, remap, names, label_list, filler=None):
    """Per transcript token, the (B, I) class pairs of every phoneme whose OUTPUT name (the merge-map back-mapping `remap` / `names`
    that Labeler._names_for builds) equals the token.  -> (alternatives, None), or (None, reason) when a token matches no phoneme
    or more than MAX_ALTERNATIVES of them.  filler (`postprocess.filler_token`; None: none): a token of that name gets the placeholder
    pair (O, O) that wfl_align_filler asks for in a filler's row."""
    pairs = class_pairs(label_list)
    by_name = {}
    for p, ph in enumerate(table.names):
        if ph in pairs:
            by_name.setdefault(names[int(remap[p])], []).append(pairs[ph])
    out = []
    for tokn in transcript:
        if filler is not None and tokn == filler:
            out.append([(label_list.index("O"),) * 2])
            continue
        alts = by_name.get(tokn)
        if not alts:
            return None, f"token {tokn!r} matches no phoneme of the label set"
        if len(alts) > MAX_ALTERNATIVES:
            return None, f"token {tokn!r} matches {len(alts)} phonemes (at most {MAX_ALTERNATIVES})"
        out.append(alts)
    return out, None


def gap_classes(label_list, transcript):
    """O, plus B- / I- of SP and of AP when the label set has them and the transcript does not spell them (silence and breaths go
    into gaps instead of stretching the neighbouring tokens)."""
    g = [label_list.index("O")]
    for ph in PAUSES:
        if ph in transcript:
            continue
        for tag in ("B-" + ph, "I-" + ph):
            if tag in label_list:
                g.append(label_list.index(tag))
    return g


def path_segments(ids, tok, chunk_frames, chunk_offsets, chunk_clock, table: npost.LabelTable, alternatives, transcript,
                  frame_duration, fillers=None, skipped=None):
    """A path over a file's chunks (ids / tok concatenated, chunk_frames[c] valid frames each) -> [(start_s, end_s, token)], exactly
    one per transcript token, in transcript order.  skipped (viterbi_align_optional's flags of this transcript's tokens; None: no
    token may be missing): the segments are then exactly the tokens whose flag is 0, in order -- a path that lacks a token without
    the flag, or holds one with it, is the RuntimeError a path that does not spell the transcript always was.  fillers
    (viterbi_align_filler's flags of this transcript's tokens; None: none): a filler yields exactly one (start, end, name) span like
    any token's run -- its start from its first frame's offset, its end capped by the next segment -- whatever classes its frames
    carry: they are decoded as one run of a stand-in phoneme, B on the run's first frame.

    Each chunk goes through the native BIO decoder (no median filter) with that chunk's offsets and is shifted by its clock offset,
    as the free decode of Labeler.label_files.  Within a token the ids are first mapped to the token's first alternative (all of
    them share the token's output name), so the decoder sees one phoneme per run; a run that crosses a chunk seam (the next chunk
    begins with I-x of the same token) is joined into one segment.  Equal neighbouring tokens stay separate segments.  A segment's
    end is capped at the next segment's start, so the segments never overlap, and is never before its own start."""
    ids = np.asarray(ids, np.int32)
    tok = np.asarray(tok, np.int32)
    b0 = np.array([a[0][0] for a in alternatives] or [0], np.int32)
    i0 = np.array([a[0][1] for a in alternatives] or [0], np.int32)
    fill = None
    if fillers is not None and any(fillers):
        if len(fillers) != len(transcript):
            raise ValueError("one filler flag per transcript token")
        fill = np.asarray([bool(f) for f in fillers] or [False])
        stand_in = next(((int(b), int(i)) for b in np.nonzero(table.kind == 1)[0]
                         for i in np.nonzero((table.kind == 2) & (table.phon == table.phon[b]))[0]), None)
        if stand_in is None:
            raise ValueError("the label set has no phoneme with both tags")
        b0[fill[:len(b0)]], i0[fill[:len(i0)]] = stand_in
    segs = []                                            # [start, end, token index]
    pos = 0
    for Tc, offs, t0 in zip(chunk_frames, chunk_offsets, chunk_clock):
        idc = ids[pos:pos + Tc]
        tkc = tok[pos:pos + Tc]
        pos += Tc
        on = tkc >= 0
        is_b = table.kind[idc] == 1
        if fill is not None:                             # a filler's frames: B where its run opens (not where it goes on over a seam)
            opens = np.concatenate([[-1 if not (segs and Tc and segs[-1][2] == tkc[0]) else tkc[0]], tkc[:-1]]) != tkc
            is_b = np.where(on & fill[np.maximum(tkc, 0)], opens, is_b)
        canon = idc.copy()
        canon[on] = np.where(is_b[on], b0[tkc[on]], i0[tkc[on]])
        s, e, _ = npost.decode_bio_ids(canon, table, frame_duration, offs, median=0)
        prev = np.concatenate([[-1], tkc[:-1]])
        starts = np.nonzero(on & (is_b | (prev != tkc)))[0]
        if len(starts) != len(s):
            raise RuntimeError(f"path decode: {len(s)} segments for {len(starts)} token runs")
        for j, f in enumerate(starts):
            k = int(tkc[f])
            if f == 0 and segs and segs[-1][2] == k:     # the token's run continues from the previous chunk
                segs[-1][1] = float(e[j]) + t0
            else:
                segs.append([float(s[j]) + t0, float(e[j]) + t0, k])
    if skipped is None:
        want = list(range(len(transcript)))
    else:
        if len(skipped) != len(transcript):
            raise ValueError("one skipped flag per transcript token")
        want = [k for k, f in enumerate(skipped) if not int(f)]
    if [g[2] for g in segs] != want:
        raise RuntimeError("the path does not spell the transcript")
    for j, g in enumerate(segs):
        if j + 1 < len(segs):                            # the decoder closes a run at the NEXT run's first frame (its end offset):
            g[1] = min(g[1], segs[j + 1][0])             # keep the segments from overlapping
        g[1] = max(g[1], g[0])                           # a one-frame run at a chunk's end closes on its own frame's end offset
    return [(a, b, transcript[k]) for a, b, k in segs]


def windows_feasible(T, windows, min_frames=None) -> bool:
    """Whether some path of a T-frame clip opens every token inside its window, i.e. whether the windowed search will NOT report
    STATUS_INFEASIBLE.  Tokens open at strictly increasing frames and nothing else constrains them (a token may be one frame long,
    gaps may be empty), so the earliest feasible start of each token decides: e_k = max(lo_k, e_{k-1} + 1) <= min(hi_k, T - 1).
    min_frames (per token; None: all 1): token k occupies at least D_k frames, so e_k = max(lo_k, e_{k-1} + D_{k-1}) <= hi_k and the
    last run ends inside the clip, e_{N-1} + D_{N-1} <= T -- for every D_k == 1 the rule above."""
    w = np.asarray(windows, np.int64).reshape(-1, 2)
    d = np.ones(len(w), np.int64) if min_frames is None else np.asarray(min_frames, np.int64).reshape(-1)
    if len(d) != len(w):
        raise ValueError("one minimum duration per window")
    e, prev = 0, 0                                       # e_{k-1} + D_{k-1}: the first frame the next token may open at
    for (lo, hi), dk in zip(w, d):
        e = max(int(lo), e + prev)
        if e > int(hi) or e + int(dk) > int(T):
            return False
        prev = int(dk)
    return True


def optional_flags(transcript, spec):
    """`postprocess.optional_tokens` -> a bool per transcript token for viterbi_align_optional.  spec: "*" (every token), or output
    names -- the transcript's own tokens -- in a list; a name the transcript lacks marks nothing."""
    if isinstance(spec, str):
        if spec != "*":
            raise ValueError("optional_tokens is a list of token names, or '*'")
        return [True] * len(transcript)
    names = set(spec)
    return [t in names for t in transcript]


def filler_flags(transcript, name):
    """`postprocess.filler_token` -> a bool per transcript token for viterbi_align_filler: the tokens equal to `name`."""
    return [t == name for t in transcript]


def collapse_fillers(transcript, name):
    """-> (the transcript with every run of adjacent fillers merged into one, how many tokens that took away)."""
    out = [t for j, t in enumerate(transcript) if not (t == name and j and transcript[j - 1] == name)]
    return out, len(transcript) - len(out)


def filler_segments(span, free_segments):
    """What a filler's span (start_s, end_s, ...) holds of the file's own free decode: every free segment that overlaps the span by
    more than nothing, clipped to it, in time order.  A span without any is empty."""
    a, b = float(span[0]), float(span[1])
    out = [(max(float(s), a), min(float(e), b), ph) for s, e, ph in free_segments if min(float(e), b) - max(float(s), a) > 0.0]
    return sorted(out, key=lambda g: (g[0], g[1]))


def min_frames_needed(flags) -> int:
    """The frames a transcript with these optional flags needs to have a path (fewer: STATUS_INFEASIBLE): at most one token is
    skipped between two kept ones, so a maximal run of r optional tokens can lose ceil(r / 2) of them -- N minus that, summed over
    the runs, and at least one frame."""
    need, run = len(flags), 0
    for f in list(flags) + [False]:
        if f:
            run += 1
        else:
            need -= (run + 1) // 2
            run = 0
    return max(need, 1)


def min_frames_for(transcript, spec, frame_duration):
    """The minimum duration of every transcript token in frames (`postprocess.min_duration`) -> [int] for viterbi_align's
    min_frames.  spec: a number of seconds for every token, or a mapping {token name: seconds, "default": seconds} (names are the
    transcript's own tokens, i.e. output names; "default", when absent 0, serves the others).  seconds -> max(1, ceil(seconds /
    frame_duration - 1e-9)) frames; more than MAX_MIN_FRAMES of them is a ValueError."""
    if isinstance(spec, (tuple, list)):                  # (the normalised, hashable form PostOptions carries)
        spec = dict(spec)
    table = spec if isinstance(spec, dict) else {"default": spec}

    def frames(seconds):
        n = max(1, int(np.ceil(float(seconds) / frame_duration - 1e-9)))
        if n > MAX_MIN_FRAMES:
            raise ValueError(f"a minimum duration of {seconds} s is {n} frames, more than the {MAX_MIN_FRAMES} the search holds")
        return n
    by_name = {name: frames(sec) for name, sec in table.items()}
    default = by_name.get("default", 1)
    return [by_name[t] if t != "default" and t in by_name else default for t in transcript]


def draft_windows(draft_segments, chunk_frames, chunk_clock, tolerance_s, frame_duration):
    """Start windows of a draft's tokens on the rows of a file's concatenated logits (chunk c: chunk_frames[c] rows, its first at
    time chunk_clock[c] of the file) -> [(lo, hi)] per draft segment (start_s, ...).

    A start time goes to a row THROUGH THE CHUNK CLOCK: its chunk is the last one whose clock is at or before the time (the first
    chunk for an earlier time), the row inside it the nearest frame -- frame f spans [f, f + 1) frame durations from the chunk's
    clock, as path_segments writes a start at (f + offset) frame durations, so the frame whose centre is nearest is
    floor((t - clock) / frame_duration) -- kept inside the chunk.  (A .lab carries times truncated to 100 ns; a thousandth of a frame
    is added before the floor.)  A division of the file time by the frame duration would drift off the rows wherever a chunk's clock
    is no multiple of it.  lo / hi are the row -+ ceil(tolerance_s / frame_duration), clipped to the file's rows; a tolerance of 0
    pins the row."""
    frames = np.asarray(chunk_frames, np.int64).reshape(-1)
    clock = np.asarray(chunk_clock, np.float64).reshape(-1)
    if len(frames) != len(clock) or not len(frames):
        raise ValueError("one clock value per chunk, at least one chunk")
    first_row = np.concatenate([[0], np.cumsum(frames)[:-1]])
    T = int(frames.sum())
    tol = int(np.ceil(float(tolerance_s) / frame_duration - 1e-9))
    out = []
    for seg in draft_segments:
        t = float(seg[0])
        c = max(int(np.searchsorted(clock, t, side="right")) - 1, 0)
        f = int(np.floor((t - clock[c]) / frame_duration + 1e-3))
        row = int(first_row[c]) + min(max(f, 0), max(int(frames[c]) - 1, 0))
        out.append((max(row - tol, 0), min(row + tol, T - 1)))
    return out


def read_draft(path):
    """The draft .lab of a file -> [(start_s, end_s, label)]: phonotactics.read_lab, the package's HTK reader."""
    from .phonotactics import read_lab
    return read_lab(path)


def with_end_pauses(free_segments, aligned, transcript):
    """The reference's rule for the ends (/root/reference/infer.py:312-319): without SP / AP in the transcript, the freely decoded
    SP / AP segments that end at or before the first aligned start or begin at or after the last aligned end are kept."""
    if "SP" not in transcript and "AP" not in transcript and aligned:
        before = [s for s in free_segments if s[2] in PAUSES and s[1] <= aligned[0][0]]
        after = [s for s in free_segments if s[2] in PAUSES and s[0] >= aligned[-1][1]]
        return before + aligned + after
    return aligned


# ------------------------------------------------------------------------------------------------------------- alignment scores
class TokenScore(NamedTuple):
    token: str
    start_s: float          # the token's segment, as in the .lab
    end_s: float
    posterior: float        # posterior occupancy of the frames Viterbi gave the token (alignment_posteriors' tok_post)
    start_sd_s: float       # posterior standard deviation of the token's start, seconds on the .lab clock
    start_shift_s: float    # posterior mean of the start minus Viterbi's start, seconds on the .lab clock


class FileScore(NamedTuple):
    path_log_posterior: float    # score - logz, <= 0; 0 means "the only plausible path"
    mean_frame_logprob: float    # score / n_frames
    mean_frame_logz: float       # logz / n_frames: comparable between transcripts of one file (the better transcript is higher)
    min_posterior: float         # the weakest token's posterior (1 for an empty transcript)
    tokens: List[TokenScore]


def file_score(score, logz, n_frames, tok_post, start_mean, start_sd, segments, frame_duration):
    """One file's FileScore from viterbi_align's score, alignment_posteriors' outputs for the file (host values) and the file's
    aligned segments [(start_s, end_s, token)], one per transcript token in order (path_segments).  frame_duration: the .lab clock
    (postprocess.FRAME_DURATION) that turns the frame figures into seconds."""
    tok_post, start_mean, start_sd = (np.asarray(a, np.float64).reshape(-1) for a in (tok_post, start_mean, start_sd))
    if not len(tok_post) == len(start_mean) == len(start_sd) == len(segments):
        raise ValueError("one posterior, start mean and start deviation per aligned segment")
    score, logz, n = float(score), float(logz), max(int(n_frames), 1)
    toks = [TokenScore(str(ph), float(s), float(e), float(p), float(sd) * frame_duration, float(mu) * frame_duration)
            for (s, e, ph), p, mu, sd in zip(segments, tok_post, start_mean, start_sd)]
    return FileScore(score - logz, score / n, logz / n, float(tok_post.min()) if len(tok_post) else 1.0, toks)


# ------------------------------------------------------------------------------------------------------------- transcript edits
def substitute_output_names(sub_names, table: npost.LabelTable, remap, names):
    """The output name of every substitute of substitute_table, through the merge-map back-mapping (`remap` / `names` of
    Labeler._names_for) that token_alternatives uses."""
    out_of = {ph: names[int(remap[p])] for p, ph in enumerate(table.names)}
    return [out_of.get(ph, ph) for ph in sub_names]


def token_edits(edits, segments, sub_out_names):
    """One file's TokenEdit rows from its rows of edit_scores' `edits` [tokens, P + 1] (host values) and its aligned segments
    [(start_s, end_s, token)].  Substitutes whose output name is the token's own are skipped; of several substitutes with one output
    name (a merge map) the best one stands for the name, so best and second are two different names."""
    edits = np.asarray(edits, np.float64).reshape(len(segments), -1)
    if edits.shape[1] != len(sub_out_names) + 1:
        raise ValueError("one column per substitute and one for the deletion")
    rows = []
    for k, (s, e, tokn) in enumerate(segments):
        by_name = {}
        for p, name in enumerate(sub_out_names):
            if name != tokn and edits[k, p] > by_name.get(name, -np.inf):
                by_name[name] = float(edits[k, p])
        order = sorted(by_name.items(), key=lambda kv: -kv[1])[:2]      # (stable: the table's order decides a tie)
        order += [("", -np.inf)] * (2 - len(order))
        dele = float(edits[k, -1])
        rows.append(TokenEdit(k, str(tokn), float(s), float(e), order[0][0], order[0][1], order[1][0], order[1][1], dele,
                              int(max(order[0][1], dele) > 0)))
    return rows


# -------------------------------------------------------------------------------------------------------- transcript insertions
def place_insertions(ins, segments, sub_out_names):
    """One file's PlaceInsertion rows from its N + 1 rows of insertion_scores' `ins` (host values) and its N aligned segments
    [(start_s, end_s, token)].  Of several substitutes with one output name (a merge map) the best one stands for the name, so best
    and second are two different names.  A substitute equal to a neighbour is not skipped: a doubled vowel is a real hypothesis."""
    n = len(segments)
    ins = np.asarray(ins, np.float64).reshape(n + 1, -1)
    if ins.shape[1] != len(sub_out_names):
        raise ValueError("one column per substitute")
    rows = []
    for j in range(n + 1):
        by_name = {}
        for p, name in enumerate(sub_out_names):
            if name not in by_name or ins[j, p] > by_name[name]:
                by_name[name] = float(ins[j, p])
        order = sorted(by_name.items(), key=lambda kv: -kv[1])[:2]      # (stable: the table's order decides a tie)
        order += [("", -np.inf)] * (2 - len(order))
        at = float(segments[j - 1][1]) if j else (float(segments[0][0]) if n else 0.0)
        rows.append(PlaceInsertion(j, str(segments[j - 1][2]) if j else "", str(segments[j][2]) if j < n else "", at, order[0][0],
                                   order[0][1], order[1][0], order[1][1], int(order[0][1] > 0)))
    return rows


# -------------------------------------------------------------------------------------------------------------- skipped tokens
def skipped_tokens(skipped, segments, transcript):
    """One file's SkippedToken rows from its tokens' `skipped` flags (viterbi_align_optional; host values) and its aligned segments
    [(start_s, end_s, token)], one per kept token in order (path_segments with the same flags)."""
    flags = [int(f) for f in skipped]
    if len(flags) != len(transcript) or len(segments) != flags.count(0):
        raise ValueError("one flag per transcript token and one segment per kept token")
    seg_of, j = {}, 0
    for k, f in enumerate(flags):
        if not f:
            seg_of[k] = segments[j]
            j += 1
    rows = []
    for k, f in enumerate(flags):
        if f:
            prev = max((q for q in seg_of if q < k), default=None)
            nxt = min((q for q in seg_of if q > k), default=None)
            at = float(seg_of[nxt][0]) if nxt is not None else (float(segments[-1][1]) if segments else 0.0)
            rows.append(SkippedToken(k, str(transcript[k]), str(transcript[prev]) if prev is not None else "",
                                     str(transcript[nxt]) if nxt is not None else "", at))
    return rows


# ------------------------------------------------------------------------------------------------------- optional tokens' scores
def optional_token_scores(optional, skipped, keep_post, segments, transcript):
    """One file's OptionalTokenScore rows, one per optional token of the transcript in order: the transcript's flags
    (optional_flags), the path's `skipped` flags and optional_posteriors' keep_post for the file (host values, one per transcript
    token) and its aligned segments, one per kept token (as skipped_tokens takes them)."""
    keep_post = np.asarray(keep_post, np.float64).reshape(-1)
    flags = [int(f) for f in skipped]
    if not len(optional) == len(flags) == len(keep_post) == len(transcript):
        raise ValueError("one optional flag, one skipped flag and one keep posterior per transcript token")
    at = {r.index: r.at_s for r in skipped_tokens(flags, segments, transcript)}
    rows, j = [], 0
    for k, f in enumerate(flags):
        if f:
            start, end = at[k], at[k]
        else:
            start, end = float(segments[j][0]), float(segments[j][1])
            j += 1
        if optional[k]:
            rows.append(OptionalTokenScore(k, str(transcript[k]), not f, float(keep_post[k]), start, end))
    return rows


# ------------------------------------------------------------------------------------------------------- filler tokens' scores
def filler_scores(spans, tok_post, start_mean, start_sd, end_mean, end_sd, frame_duration):
    """One file's FillerScore rows, one per FillerSpan in order, from filler_posteriors' outputs for the file (host values, one per
    transcript token).  frame_duration: the .lab clock that turns the frame figures into seconds."""
    cols = [np.asarray(a, np.float64).reshape(-1) for a in (tok_post, start_mean, start_sd, end_mean, end_sd)]
    if len({len(c) for c in cols}) != 1:
        raise ValueError("one posterior and one pair of start and end moments per transcript token")
    rows = []
    for sp in spans:
        if not 0 <= sp.index < len(cols[0]):
            raise ValueError("a filler span's index lies outside the transcript")
        p, smu, ssd, emu, esd = (float(c[sp.index]) for c in cols)
        rows.append(FillerScore(sp.index, sp.start_s, sp.end_s, sp.frames, p, smu * frame_duration, ssd * frame_duration,
                                emu * frame_duration, esd * frame_duration))
    return rows


# ---------------------------------------------------------------------------------------- token durations under a duration prior
def token_durations(tokens, frames, rows, table, tok_post, start_mean, start_sd, end_mean, end_sd, frame_duration):
    """One file's TokenDuration rows, one per transcript token in order, from duration_prior_posteriors' outputs for the file (host
    values, one per token).  tokens: the file's TokenScore rows (file_score); frames: the frames of every token's run; rows, table:
    the tokens' rows of the duration table and the table ([rows, D + 1], as viterbi_align_duration_prior's); frame_duration: the .lab
    clock that turns the frame figures into seconds."""
    cols = [np.asarray(a, np.float64).reshape(-1) for a in (tok_post, start_mean, start_sd, end_mean, end_sd)]
    if len({len(c) for c in cols} | {len(tokens), len(frames), len(rows)}) != 1:
        raise ValueError("one token, run length, table row, posterior and pair of start and end moments per transcript token")
    table = np.asarray(table, np.float64)
    D = table.shape[1] - 1
    out = []
    for k, (t, d, r) in enumerate(zip(tokens, frames, rows)):
        d, r = int(d), int(r)
        prior = None
        if r >= 0:
            prior = float(table[r, d - 1]) if d <= D else float(table[r, D - 1]) + (d - D) * float(table[r, D])
        p, smu, ssd, emu, esd = (float(c[k]) for c in cols)
        out.append(TokenDuration(k, t.token, t.start_s, t.end_s, d, prior, p, smu * frame_duration, ssd * frame_duration,
                                 emu * frame_duration, esd * frame_duration, d + emu - smu))
    return out


# ------------------------------------------------------------------------------------------------------- pronunciation variants
VARIANT_CHARS = "(|)"       # syntax of a `{audio}.txt` under `postprocess.transcript_variants`, wherever they occur
MAX_VARIANTS = 4            # variants per group
MAX_SLOTS = 2047            # wfl_align_graph's slot cap per clip (status 2 above it)
MAX_PREDECESSORS = 8        # predecessors per slot
MAX_SPAN = 255              # a predecessor is at most this many slots back
START, UNUSED = -1, -2      # slot_pred's values that are no slot


def graph_workspace_bytes(n_frames, n_slots) -> int:
    return _workspace_bytes("wfl_align_graph_workspace_bytes", n_frames, n_slots)


def has_variants(tokens) -> bool:
    """Whether a transcript's tokens (the whitespace-separated words of a `.txt`) hold any of the three syntax characters."""
    return any(ch in tok for tok in tokens for ch in VARIANT_CHARS)


def variant_name_collisions(output_names):
    """The output names of a label set that hold one of the three syntax characters: with transcript_variants on they could not be
    spelled, so the caller that knows the model refuses them by name."""
    return sorted({n for n in output_names if any(ch in n for ch in VARIANT_CHARS)})


def parse_variants(tokens, notes=None):
    """The words of a `.txt` -> its elements, in order: a plain token is a str, a group a tuple of 2 to MAX_VARIANTS variants, each a
    tuple of tokens (the empty tuple: the group may be left out); the first variant is the transcript as written.  `(`, `|` and `)`
    are syntax wherever they occur, attached to a name or alone.  A ValueError names the place (the 1-based word) of: nesting, an
    unbalanced parenthesis, a `|` outside a group, a group with fewer than 2 distinct variants, one with more than MAX_VARIANTS.
    Duplicate variants inside a group collapse (the first stays); `notes` (a list) receives one line for each such group."""
    elements, group, current, opened = [], None, None, 0
    for place, word in enumerate(tokens, 1):
        name = ""
        for ch in list(word) + [" "]:
            if ch not in VARIANT_CHARS and ch != " ":
                name += ch
                continue
            if name:
                (current if group is not None else elements).append(name)
                name = ""
            if ch == "(":
                if group is not None:
                    raise ValueError(f"word {place}: a group inside the group opened at word {opened} (variants do not nest)")
                group, current, opened = [], [], place
            elif ch == "|":
                if group is None:
                    raise ValueError(f"word {place}: '|' outside a group")
                group.append(tuple(current))
                current = []
            elif ch == ")":
                if group is None:
                    raise ValueError(f"word {place}: ')' without a '('")
                group.append(tuple(current))
                if len(group) > MAX_VARIANTS:
                    raise ValueError(f"word {place}: the group opened at word {opened} has {len(group)} variants (at most {MAX_VARIANTS})")
                distinct = list(dict.fromkeys(group))
                if len(distinct) < 2:
                    raise ValueError(f"word {place}: the group opened at word {opened} needs at least 2 distinct variants")
                if len(distinct) < len(group) and notes is not None:
                    notes.append(f"the group opened at word {opened} repeats a variant: {len(group) - len(distinct)} dropped")
                elements.append(tuple(distinct))
                group, current = None, None
    if group is not None:
        raise ValueError(f"word {opened}: '(' is never closed")
    return elements


class TranscriptGraph(NamedTuple):
    """compile_graph's record of a transcript with variants."""
    slots: list       # the token name of every slot, in topological order: element by element, a group's variants one after the other
    preds: list       # per slot its predecessors, in order: START (-1) or earlier slots
    final: list       # per slot 0 | 1: the path may end there
    groups: list      # per group, in order: per variant its (first slot, one past its last slot); an empty variant is (k, k)
    elements: list    # parse_variants' elements

    @property
    def first(self):
        """The slots of the first-variant expansion, the transcript as written."""
        out, k, gi = [], 0, 0
        for el in self.elements:
            if isinstance(el, str):
                out.append(k)
                k += 1
            else:
                a, b = self.groups[gi][0]
                out.extend(range(a, b))
                k = self.groups[gi][-1][1]
                gi += 1
        return out

    def spelling(self, gi, v) -> str:
        a, b = self.groups[gi][v]
        return " ".join(self.slots[a:b])


def compile_graph(elements) -> TranscriptGraph:
    """parse_variants' elements -> the slots of wfl_align_graph.  A plain token's predecessors are the current frontier (at first:
    START) and it becomes the frontier; every non-empty variant of a group opens from the frontier and chains inside, and the new
    frontier is the variants' last slots, plus the old frontier for an empty variant -- order kept, entries deduplicated.  The finals
    are the last frontier.  ValueError: a transcript whose every element is a group with an empty variant (it could spell nothing),
    a slot that would need more than MAX_PREDECESSORS predecessors (runs of adjacent optional groups), a group of more than MAX_SPAN
    slots, a predecessor more than MAX_SPAN slots back."""
    if all(not isinstance(el, str) and () in el for el in elements):
        raise ValueError("every element of the transcript is a group with an empty variant: it could spell nothing")
    slots, preds, groups = [], [], []
    frontier = [START]

    def add(name, pr, where):
        if len(pr) > MAX_PREDECESSORS:
            raise ValueError(f"{where}: token {name!r} would need {len(pr)} predecessors (at most {MAX_PREDECESSORS}): too many adjacent "
                             "optional groups in front of it")
        k = len(slots)
        if any(p != START and k - p > MAX_SPAN for p in pr):
            raise ValueError(f"{where}: token {name!r} would follow a token more than {MAX_SPAN} slots back")
        slots.append(name)
        preds.append(list(pr))
        return k

    for ei, el in enumerate(elements, 1):
        where = f"element {ei}"
        if isinstance(el, str):
            frontier = [add(el, frontier, where)]
            continue
        if sum(len(v) for v in el) > MAX_SPAN:
            raise ValueError(f"{where}: a group of {sum(len(v) for v in el)} slots (at most {MAX_SPAN})")
        ranges, new = [], []
        for var in el:
            a = len(slots)
            if not var:
                new.extend(frontier)
            else:
                last = None
                for name in var:
                    last = add(name, frontier if last is None else [last], where)
                new.append(last)
            ranges.append((a, len(slots)))
        groups.append(ranges)
        frontier = list(dict.fromkeys(new))
    final = [0] * len(slots)
    for k in frontier:
        if k != START:
            final[k] = 1
    return TranscriptGraph(slots, preds, final, groups, list(elements))


def chain_graph(n):
    """(preds, final) of the chain of n slots: wfl_align's lattice as a graph."""
    return [[START if k == 0 else k - 1] for k in range(n)], [int(k == n - 1) for k in range(n)]


def _pack_graph(slot_preds, slot_final, N):
    """Per clip the predecessor lists and the final flags of its slots -> ([max(slots, 1), 8] int32, unused entries -2, and
    [max(slots, 1)] int32), rows as the token table's.  The values are not judged here: the kernel's STATUS_BAD_CLASS is."""
    if len(slot_preds) != len(N) or len(slot_final) != len(N):
        raise ValueError("slot_preds and slot_final need one entry per clip")
    total = max(int(N.sum()), 1)
    pr = np.full((total, MAX_PREDECESSORS), UNUSED, np.int64)
    fn = np.zeros(total, np.int64)
    k0 = 0
    for p, f, n in zip(slot_preds, slot_final, N):
        if len(p) != n or len(f) != n:
            raise ValueError(f"a clip with {n} slots needs {n} predecessor lists and {n} final flags")
        for k, row in enumerate(p):
            row = list(row)
            if len(row) > MAX_PREDECESSORS:
                raise ValueError(f"a slot has at most {MAX_PREDECESSORS} predecessors, got {len(row)}")
            pr[k0 + k, :len(row)] = row
        fn[k0:k0 + n] = np.asarray(f, np.int64).reshape(-1) if n else 0
        k0 += int(n)
    if min(pr.min(), fn.min()) < -2 ** 31 or max(pr.max(), fn.max()) > 2 ** 31 - 1:
        raise ValueError("predecessors and final flags are int32")
    return pr.astype(np.int32), fn.astype(np.int32)


class PackedGraph(NamedTuple):
    """pack_graph's result: the PackedClips of the slots and the uploaded predecessor and final tables of a ragged batch."""
    clips: PackedClips
    d_pred: torch.Tensor      # [max(slots, 1), 8] int32
    d_final: torch.Tensor     # [max(slots, 1)] int32


def pack_graph(logits, n_frames, slot_classes, slot_preds, slot_final, gap_classes, frame_offsets=None) -> PackedGraph:
    """Validate a ragged batch of transcript graphs and upload its tables once; pass the result as `packed=` to viterbi_align_graph
    calls over the same batch."""
    nb, T, N, F0, K0, tc, gc = _pack_clips(logits, n_frames, slot_classes, gap_classes, frame_offsets)
    pr, fn = _pack_graph(slot_preds, slot_final, N)
    dev = logits.device
    return PackedGraph(PackedClips(nb, T, N, F0, K0, torch.from_numpy(tc).to(dev), torch.from_numpy(gc).to(dev)),
                       torch.from_numpy(pr).to(dev), torch.from_numpy(fn).to(dev))


def viterbi_align_graph(logits, n_frames, slot_classes, slot_preds, slot_final, gap_classes, o_id, frame_offsets=None, stream=None,
                        packed=None):
    """Forced alignment of a ragged batch of transcript GRAPHS on the GPU (wfl_align_graph): the search chooses among the variants.

    slot_classes  per clip, per slot: 1..4 (B, I) class pairs, as viterbi_align's token_classes
    slot_preds    per clip, per slot: its predecessors in order of preference, START (-1) or clip-local slots k - MAX_SPAN <= j < k,
                  at most MAX_PREDECESSORS (compile_graph's preds; chain_graph's for a plain transcript)
    slot_final    per clip, per slot: 0 | 1, the path may end in the slot
    packed        pack_graph(...) of these same arguments, to pack and upload the tables once for several calls (default: packed here)
    the others    as viterbi_align's
    -> (ids, tok, score, status, taken): viterbi_align's four, tok the clip-local slot, and taken [slots] int32, 1 for a slot the
    path visits, in the order of the clips' slots.  STATUS_INFEASIBLE: no path through the graph fits the frames; STATUS_OVER_CAP:
    more than MAX_SLOTS slots; STATUS_BAD_CLASS also for a malformed graph (include/wfl_asr.h).  A clip with status != 0 has
    taken = 0.  On chain_graph's lists ids, tok and status are viterbi_align's."""
    if packed is None:
        packed = pack_graph(logits, n_frames, slot_classes, slot_preds, slot_final, gap_classes, frame_offsets)
    clips, d_pr, d_fn = packed
    dev, rows, nb, ntok = logits.device, logits.shape[0], clips.nb, int(clips.N.sum())
    ids = torch.empty(rows, dtype=torch.int32, device=dev)
    tok = torch.empty(rows, dtype=torch.int32, device=dev)
    score = torch.empty(max(nb, 1), dtype=torch.float32, device=dev)
    status = torch.empty(max(nb, 1), dtype=torch.int32, device=dev)
    taken = torch.empty(max(ntok, 1), dtype=torch.int32, device=dev)
    _call("wfl_align_graph", logits, o_id, clips, (d_pr, d_fn), (ids, tok, score, taken, status), stream, temporaries=(d_pr, d_fn))
    return ids, tok, score[:nb], status[:nb], taken[:ntok]


def variant_choices(graph: TranscriptGraph, taken, segments, gain=None):
    """One file's VariantChoice rows, one per group in order, from the path's `taken` flags (host values, one per slot) and its
    segments [(start_s, end_s, token)], one per taken slot in order (path_segments with skipped = 1 - taken).  The chosen variant is
    the one whose slots are taken -- the empty one where none is; its time is its first segment's start to its last segment's end,
    for an empty one the time of the place: the start of the next taken slot's segment, the end of the last segment when nothing
    follows.  gain: the file's gain in nats (None: the transcript as written has no path of its own)."""
    flags = [int(f) for f in taken]
    if len(flags) != len(graph.slots) or len(segments) != sum(flags):
        raise ValueError("one flag per slot and one segment per taken slot")
    seg_of, j = {}, 0
    for k, f in enumerate(flags):
        if f:
            seg_of[k] = segments[j]
            j += 1
    rows = []
    for gi, ranges in enumerate(graph.groups):
        chosen = [v for v, (a, b) in enumerate(ranges) if b > a and all(flags[a:b])]
        empty = [v for v, (a, b) in enumerate(ranges) if b == a]
        if len(chosen) > 1 or (not chosen and (not empty or any(flags[ranges[0][0]:ranges[-1][1]]))):
            raise ValueError(f"group {gi}: the taken slots are not one variant")
        v = chosen[0] if chosen else empty[0]
        a, b = ranges[v]
        if b > a:
            start, end = float(seg_of[a][0]), float(seg_of[b - 1][1])
        else:
            nxt = min((q for q in seg_of if q >= ranges[-1][1]), default=None)
            start = end = float(seg_of[nxt][0]) if nxt is not None else (float(segments[-1][1]) if segments else 0.0)
        rows.append(VariantChoice(gi, start, end, v, graph.spelling(gi, v), graph.spelling(gi, 0), gain))
    return rows
