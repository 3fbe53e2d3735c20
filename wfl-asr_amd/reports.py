"""The side reports of a Viterbi-aligned labelling run: the files written beside the .lab files, `{stem}{suffix}` per labelled file and
`{folder stem}.tsv` per folder.  KINDS is the one table of their kinds -- REPORTS, the seven kinds that report on a chain lattice,
and behind them the kinds that came later (`variants`, of the transcript graph); everything a kind needs is in its entry, and the
callers (infer.py) loop over the table.  A kind's rows are computed in align.py (token_edits, place_insertions, skipped_tokens,
optional_token_scores, filler_scores, token_durations, variant_choices; the FillerSpan rows in Labeler._clip_label) and travel from
the search to the writer in a Reports.

A new kind: its row record and an entry of KINDS here, its row builder in align.py, and one line of the Labeler stage that puts the
rows under the kind's key (Labeler._clip_label; Labeler._search_variants for `variants`)."""
import os
from typing import Callable, NamedTuple


# ------------------------------------------------------------------------------------------------------------------ the row records
class TokenEdit(NamedTuple):
    index: int
    token: str
    start_s: float
    end_s: float
    best: str               # output name of the best substitute ("" when the table holds none for this token)
    best_ratio: float       # its log likelihood ratio against the transcript as written (-inf: none)
    second: str
    second_ratio: float
    deletion_ratio: float   # the same for the transcript without the token
    flag: int               # 1 when the largest of the three ratios is > 0: an edit explains the audio better

    @property
    def largest(self) -> float:
        return max(self.best_ratio, self.second_ratio, self.deletion_ratio)


class PlaceInsertion(NamedTuple):
    index: int              # the place: 0 .. N, in front of token `index` (N: behind the last token)
    after: str              # the neighbour tokens' names, "" at the ends
    before: str
    at_s: float             # the boundary of the Viterbi path there: the end of token index - 1, for index 0 the start of token 0
    best: str               # output name of the best phoneme to insert ("" when the table is empty)
    best_ratio: float       # its log likelihood ratio against the transcript as written (-inf: none, or no path)
    second: str
    second_ratio: float
    flag: int               # 1 when best_ratio > 0: a token inserted here explains the audio better


class SkippedToken(NamedTuple):
    index: int              # the token's index in the transcript
    token: str
    after: str              # the kept tokens around the place, "" at the ends
    before: str
    at_s: float             # the place: the start of the next kept token's segment, the end of the last segment when nothing follows


class OptionalTokenScore(NamedTuple):
    index: int              # the token's index in the transcript
    token: str
    kept: bool              # the best path holds the token
    keep_posterior: float   # optional_posteriors' keep_post: the posterior probability that the token is present
    start_s: float          # a kept token's segment; for a skipped one both are the place's time (SkippedToken.at_s)
    end_s: float

    @property
    def confidence(self) -> float:
        """The posterior mass behind the decision the best path took."""
        return self.keep_posterior if self.kept else 1.0 - self.keep_posterior

    @property
    def doubt(self) -> bool:
        """The opposite decision has more posterior mass than the one the best path took."""
        return self.confidence < 0.5


class FillerSpan(NamedTuple):
    index: int              # the filler's index in the transcript (after collapse_fillers)
    start_s: float          # its span on the .lab clock
    end_s: float
    frames: int             # the frames of its run
    names: tuple            # the names of the free segments the span holds (filler_segments), in time order


class FillerScore(NamedTuple):
    index: int              # the filler's index in the transcript (after collapse_fillers)
    start_s: float          # its span on the .lab clock
    end_s: float
    frames: int             # the frames of its run
    posterior: float        # filler_posteriors' tok_post: the posterior that the span's frames belong to the filler
    start_shift_s: float    # posterior mean of the span's start minus Viterbi's, seconds on the .lab clock
    start_sd_s: float       # posterior standard deviation of the start, seconds
    end_shift_s: float      # the same for the span's end (filler_posteriors' end_mean / end_sd)
    end_sd_s: float


class TokenDuration(NamedTuple):
    index: int              # the token's index in the transcript
    token: str
    start_s: float          # its run on the .lab clock
    end_s: float
    frames: int             # the frames of its run
    log_prior: float        # the table's L(frames) of the token's row: weight * log P(frames | phoneme); None for a token without a row
    posterior: float        # duration_prior_posteriors' tok_post: the posterior that the run's frames belong to the token
    start_shift_s: float    # posterior mean of the run's start minus the search's, seconds on the .lab clock
    start_sd_s: float       # posterior standard deviation of the start, seconds
    end_shift_s: float      # the same for the run's end
    end_sd_s: float
    expected_frames: float  # frames + end_mean - start_mean: the posterior mean of the token's length (exact, by linearity)


class VariantChoice(NamedTuple):
    index: int              # the group's index among the transcript's groups
    start_s: float          # the chosen variant on the .lab clock; for an empty one both are the time of the place
    end_s: float
    choice: int             # the chosen variant's number, 0 the transcript as written
    spelling: str           # its tokens ("" for the empty variant)
    written: str            # the first variant's tokens
    gain: float             # the file's gain in nats: the graph's score minus the score of the transcript as written (None: that has no path)


# ------------------------------------------------------------------------------------------------------------- a row's cells, as text
def _edit_cells(r: TokenEdit):
    return [str(r.index), r.token, f"{r.start_s:.7f}", f"{r.end_s:.7f}", r.best, f"{r.best_ratio:.6g}", r.second,
            f"{r.second_ratio:.6g}", f"{r.deletion_ratio:.6g}", str(r.flag)]


def _insertion_cells(r: PlaceInsertion):
    return [str(r.index), r.after, r.before, f"{r.at_s:.7f}", r.best, f"{r.best_ratio:.6g}", r.second, f"{r.second_ratio:.6g}",
            str(r.flag)]


def _skipped_cells(r: SkippedToken):
    return [str(r.index), r.token, r.after, r.before, f"{r.at_s:.7f}"]


def _optional_cells(r: OptionalTokenScore):
    return [str(r.index), r.token, "kept" if r.kept else "skipped", f"{r.keep_posterior:.6f}", f"{r.start_s:.7f}", f"{r.end_s:.7f}",
            "1" if r.doubt else "0"]


def _filler_cells(r: FillerSpan):
    return [str(r.index), f"{r.start_s:.7f}", f"{r.end_s:.7f}", str(r.frames), " ".join(str(n) for n in r.names)]


def _filler_score_cells(r: FillerScore):
    return [str(r.index), f"{r.start_s:.7f}", f"{r.end_s:.7f}", str(r.frames), f"{r.posterior:.6f}", f"{r.start_shift_s:.7f}",
            f"{r.start_sd_s:.7f}", f"{r.end_shift_s:.7f}", f"{r.end_sd_s:.7f}"]


def _duration_cells(r: TokenDuration):
    return [str(r.index), r.token, f"{r.start_s:.7f}", f"{r.end_s:.7f}", str(r.frames),
            "none" if r.log_prior is None else f"{r.log_prior:.6f}", f"{r.posterior:.6f}", f"{r.start_shift_s:.7f}", f"{r.start_sd_s:.7f}",
            f"{r.end_shift_s:.7f}", f"{r.end_sd_s:.7f}", f"{r.expected_frames:.4f}"]


def _variant_cells(r: VariantChoice):
    return [str(r.index), f"{r.start_s:.7f}", f"{r.end_s:.7f}", str(r.choice), r.spelling, r.written,
            "none" if r.gain is None else f"{r.gain:.6g}"]


# ------------------------------------------------------------------------------------------------------------------------ the table
class Kind(NamedTuple):
    key: str                # the name of the kind: Reports.rows' key, and the place of its list in Labeler.label_files' result
    enabled: Callable       # resolved options (options.PostOptions) -> whether a run collects and writes the kind
    suffix: str             # `{stem}{suffix}` beside a file's .lab: one line per row, in the rows' order
    stem: str               # `{stem}.tsv` of a folder (`{stem}.rank{r}.tsv` of one process among several)
    what: str               # "{what} saved to: ..." / "{what} of the folder saved to: ..."
    header: str             # the column names; the folder file has `file` in front
    cells: Callable         # row -> its cells, as text
    keep: Callable = None   # the folder file lists the rows for which keep(row) holds (None: every row) ...
    order: Callable = None  # ... by order(row), ascending; ties, and None, in the files' and the rows' order
    missing: str = None     # "{path}: {missing} (the file was not Viterbi-aligned)", None: no line


REPORTS = {k.key: k for k in (
    # per transcript token; the folder file: every flagged token by its largest ratio, descending
    Kind("edits", lambda o: o.align_edits, ".edits.tsv", "transcript_edits", "Transcript edits",
         "index\ttoken\tstart_s\tend_s\tbest\tbest_log_ratio\tsecond\tsecond_log_ratio\tdeletion_log_ratio\tflag", _edit_cells,
         keep=lambda r: r.flag, order=lambda r: -r.largest, missing="no transcript edits"),
    # per place of the transcript; the folder file: every flagged place by its best ratio, descending
    Kind("insertions", lambda o: o.align_insertions, ".insertions.tsv", "transcript_insertions", "Transcript insertions",
         "index\tafter\tbefore\tat_s\tbest\tbest_log_ratio\tsecond\tsecond_log_ratio\tflag", _insertion_cells,
         keep=lambda r: r.flag, order=lambda r: -r.best_ratio, missing="no transcript insertions"),
    # per token the path left out
    Kind("skipped", lambda o: o.optional_tokens is not None, ".skipped.tsv", "skipped_tokens", "Skipped tokens",
         "index\ttoken\tafter\tbefore\tat_s", _skipped_cells),
    # per optional token of the transcript; the folder file: the least confident decision first
    Kind("optional", lambda o: o.optional_scores, ".optional.tsv", "optional_scores", "Optional-token scores",
         "index\ttoken\tdecision\tkeep_posterior\tstart_s\tend_s\tdoubt", _optional_cells,
         order=lambda r: r.confidence, missing="no optional-token scores"),
    # per filler of the transcript
    Kind("fillers", lambda o: o.filler_token is not None, ".fillers.tsv", "filler_spans", "Filler spans",
         "index\tstart_s\tend_s\tframes\tnames", _filler_cells),
    # per filler of the transcript; the folder file: the lowest occupancy posterior first.  No flag, no threshold: the order is the
    # list to check
    Kind("filler_scores", lambda o: o.filler_scores, ".filler_scores.tsv", "filler_scores", "Filler scores",
         "index\tstart_s\tend_s\tframes\tposterior\tstart_shift_s\tstart_sd_s\tend_shift_s\tend_sd_s", _filler_score_cells,
         order=lambda r: r.posterior, missing="no filler scores"),
    # per transcript token; the folder file: every token that has a prior row, the lowest log_prior first (the length the prior finds
    # least probable).  No flag, no threshold: the order is the list to check
    Kind("durations", lambda o: o.duration_prior_scores, ".durations.tsv", "token_durations", "Token durations",
         "index\ttoken\tstart_s\tend_s\tframes\tlog_prior\tposterior\tstart_shift_s\tstart_sd_s\tend_shift_s\tend_sd_s\texpected_frames",
         _duration_cells, keep=lambda r: r.log_prior is not None, order=lambda r: r.log_prior, missing="no duration-prior scores"),
)}

# REPORTS is the table of the seven kinds that report on a chain lattice; KINDS is the whole table, those and the kinds that came
# after them.  Everything below, and every caller, looks a kind up in KINDS.
KINDS = {**REPORTS, **{k.key: k for k in (
    # per group of a transcript with variants; the folder file: every group whose choice is not the transcript as written, the file
    # with the largest gain first (a file without a gain last)
    Kind("variants", lambda o: getattr(o, "transcript_variants", False), ".variants.tsv", "transcript_variants", "Transcript variants",
         "index\tstart_s\tend_s\tvariant\tspelling\twritten\tgain_nats", _variant_cells,
         keep=lambda r: r.choice != 0, order=lambda r: float("inf") if r.gain is None else -r.gain),
)}}


def file_text(key, rows) -> str:
    """`{stem}{suffix}` of one file: the header, then one line per row (an empty report is its header alone)."""
    kind = KINDS[key]
    return "".join(line + "\n" for line in [kind.header] + ["\t".join(kind.cells(r)) for r in rows])


def folder_rows(key, per_file):
    """per_file: [(file name, rows)] -> the rows of the kind's folder file as [(file name, row)]: Kind.keep, Kind.order."""
    kind = KINDS[key]
    flat = [(name, r) for name, rows in per_file for r in rows if kind.keep is None or kind.keep(r)]
    return flat if kind.order is None else sorted(flat, key=lambda nr: kind.order(nr[1]))      # (stable: the descending ones negate)


def folder_text(key, per_file) -> str:
    """`{folder stem}.tsv`: folder_rows, the file's name in front of the row's own columns."""
    kind = KINDS[key]
    lines = ["file\t" + kind.header] + ["\t".join([name] + kind.cells(r)) for name, r in folder_rows(key, per_file)]
    return "".join(line + "\n" for line in lines)


def file_path(key, lab_path) -> str:
    return os.path.splitext(lab_path)[0] + KINDS[key].suffix


class Reports:
    """What one labelling run collects beside segments and scores: per enabled kind {file index: rows} for the files that were
    Viterbi-aligned that way (`rows`, in REPORTS' order), and {file index: [DraftMove]} for the files aligned inside their draft's
    windows (`moves`)."""

    def __init__(self, keys=()):
        self.rows = {key: {} for key in keys}
        self.moves = {}

    @classmethod
    def for_options(cls, opts):
        return cls(key for key, kind in KINDS.items() if kind.enabled(opts))

    def take(self, fi, rows_of, moves=None):
        """File fi's rows by kind (a kind that is not enabled is dropped) and its draft moves (None: none)."""
        for key, rows in rows_of.items():
            if key in self.rows:
                self.rows[key][fi] = rows
        if moves is not None:
            self.moves[fi] = moves

    def named(self, key, names):
        """[(names[fi], rows)] of the kind, in the files' order: what folder_text takes."""
        return [(names[fi], rows) for fi, rows in sorted(self.rows[key].items())]
