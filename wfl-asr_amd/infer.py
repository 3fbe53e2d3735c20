"""The inference surface of WFL-ASR on the MI355X path: same functions, arguments, files and `.lab` output as
/root/reference/infer.py, with the per-file model rebuild and the B=1 forwards replaced by one resident model and a
batched loop over 30 s work items.

  infer_audio / infer_folder   signatures of infer.py:186-191 / 330-332
  Labeler                      the batched loop: one model load (the reference reloads per file, infer.py:205-208),
                               every clip <= 30 s and every 30 s chunk of a longer file is one batch row; rows of many
                               files share a forward; `lang_id=None` averages logits/offsets over all languages
                               inside the library (encoder runs once; infer.py:146-156, 266-276)
  options.resolve              the post-processing options of a request (align, decode, the scores, the phone bigram, the draft): resolved
                               once per request into a PostOptions record, and once before any model is loaded (options.py)
  deviations (documented in DESIGN.md): no `.wfl_cache` (infer.py:223-229), `--sample/--top-k/--top-p/--temperature`
  are validated but have no effect (their results are overwritten in the reference too, infer.py:283-297), a single
  file with `-o .` writes `<stem>.lab` instead of overwriting the input WAV (infer.py:410-411, utils.py:77), and
  `--device cpu` is refused (no CPU path).
"""
from __future__ import annotations

import math
import os
import sys
from concurrent.futures import ThreadPoolExecutor
from typing import NamedTuple

import numpy as np
import torch
import yaml

from . import align as AL
from . import audio as A
from . import decode as DC
from . import native_post as npost
from . import postprocess as pp
from . import reports as R
from ._lib import back_to_back
from .options import (ALIGN_MODES, DECODE_MODES, PostOptions, filler_token_collision, parse_min_duration, resolve,
                      unknown_optional_tokens)
from .tagger import BIOPhonemeTagger, raise_on_status

frame_duration = pp.FRAME_DURATION
MAX_SEGMENT_DURATION = pp.MAX_SEGMENT_DURATION
CHUNK_SAMPLES = int(MAX_SEGMENT_DURATION * 16000)     # at 16 kHz; a Labeler's own work-item length is `chunk_samples` (its config's rate)


def load_config(config_path="config.yaml"):
    with open(config_path, "r") as f:
        return yaml.safe_load(f)


def _worker_threads(n_tasks=16):
    """Threads of a pool of host workers (the native loaders release the GIL)."""
    return max(1, min(16, os.cpu_count() or 1, n_tasks))


def pick_device(device="cuda") -> torch.device:
    """The HIP device this process labels on.  An explicit index wins; a bare "cuda" means cuda:LOCAL_RANK under a
    one-process-per-GPU launcher (torchrun sets LOCAL_RANK and WORLD_SIZE) and the current device otherwise."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("this build labels on MI355X only: --device must be cuda[:N] (there is no CPU path)")
    if dev.index is not None:
        return dev
    if int(os.environ.get("WORLD_SIZE", "1")) > 1 and "LOCAL_RANK" in os.environ:
        return torch.device("cuda", int(os.environ["LOCAL_RANK"]))
    return torch.device("cuda", torch.cuda.current_device())


class Labeler:
    """Model + sidecar files loaded once; `label_files` runs the batched hot loop."""

    def __init__(self, config_path, checkpoint_path, device="cuda", batch_size=None, use_graph=False):
        self.config = load_config(config_path) if isinstance(config_path, (str, os.PathLike)) else config_path
        if torch.device(device).type == "cuda" and not torch.cuda.is_available():
            raise RuntimeError("no ROCm device visible")
        self.device = pick_device(device)
        torch.cuda.set_device(self.device)       # weights, workspaces, streams and pinned staging all belong to this device
        self.sr = int(self.config["data"]["sample_rate"])
        enc = str(self.config["model"]["encoder_type"]).lower()
        if self.sr != 16000 and enc not in ("none", "null"):
            raise ValueError("both encoders are 16 kHz models (config data.sample_rate must be 16000)")
        # every file is resampled to the config's rate and cut into 30 s work items (infer.py:19-28, 218-220); the mel front-end of
        # `encoder_type: none` runs at that rate (its hop is int(frame_duration * sample_rate))
        self.chunk_samples = int(MAX_SEGMENT_DURATION * self.sr)
        save_dir = self.config["output"]["save_dir"]
        self.labels = pp.load_phoneme_list(os.path.join(save_dir, "phonemes.txt"))
        langs_path = os.path.join(save_dir, "langs.txt")
        self.lang2id = pp.load_langs(langs_path) if os.path.exists(langs_path) else {}
        mm_path = os.path.join(save_dir, "phoneme_merge_map.json")
        self.merge_map = pp.load_phoneme_merge_map(mm_path) if os.path.exists(mm_path) else None
        self.model = BIOPhonemeTagger(self.config, self.labels, device=self.device, any_rate=True)   # (`none`: the config's own rate)
        if isinstance(checkpoint_path, dict):
            state_dict = checkpoint_path
        else:
            state_dict = torch.load(checkpoint_path, map_location="cpu", weights_only=True)
        self.model.load_state_dict(state_dict)
        self.model.to(self.device).eval()
        if self.lang2id:
            # `lang_id=None` averages over the ids langs.txt lists, in file order (infer.py:147-156, 266-276)
            self.model.set_average_languages(list(self.lang2id.values()))
        if batch_size is None:
            # rows per forward.  A BiLSTM's recurrence costs the same ~1.2 us per time step for 16 clips as for 64 (clips run in
            # groups of 16 on their own workgroups), so wide batches amortise it: default head, 64 rows 107 k audio-s/s, 16 rows 87 k
            # (DESIGN.md section 5).  A clip's tags do not depend on what shares its batch (bit-exact batch invariance).
            batch_size = int(os.environ.get("WFL_BATCH_SIZE", "64" if self.model.head_cfg["enable_bilstm"] else "16"))
        self.batch_size = int(batch_size)
        self.use_graph = bool(use_graph)
        self.n_inflight = self.model.batches_in_flight()   # batches on the GPU at once: stream + workspace slot each
        self._table = npost.LabelTable(self.labels)          # native BIO decode works on ids (csrc/hostpost.hip)
        self._streams = None
        self._pinned = {}                                    # dtype -> ring of flat pinned staging buffers (_pinned_ring)
        self._names_cache = {}                               # _names_for
        self._decode_table = None                            # decode.class_table(labels), built by the first grammar decode
        self._bigram_cache = {}                              # (path, switch penalty, weight) -> transition table (_bigram_table)
        self._wave_items = None                              # chunks per wave of files; None: _wave()

    # ------------------------------------------------------------------ the batched loop
    def _forward_items(self, items, lang_id, threshold):
        """items: list of float32 arrays (<= 480000 samples each) -> list of (ids[T], offsets[T,2]) numpy, in item order."""
        if self.model.encoder_type != "whisper":
            return self._forward_items_by_length(items, lang_id, threshold)
        out = [None] * len(items)
        Bs, L = self.batch_size, self.chunk_samples

        def fill(k, host):
            lens = np.zeros(Bs, dtype=np.int32)
            rows = host.numpy()                  # (a numpy row assignment is a plain memcpy, 0.2 ms per 30 s item; the same through
            for i, x in enumerate(items[k * Bs:(k + 1) * Bs]):   # torch's indexing was measured at 1-18 ms)
                n = min(len(x), L)
                rows[i, :n] = x[:n]
                lens[i] = n
            return lens

        def take(k, ids, offs):
            for i in range(min(Bs, len(items) - k * Bs)):
                out[k * Bs + i] = (ids[i].copy(), offs[i].copy())

        self._pipeline([(Bs, L, self.model.num_frames(L))] * -(-len(items) // Bs), fill, take, lang_id, threshold, graph=self.use_graph)
        return out

    def _pinned_ring(self, n, dtype, capacity):
        """n flat pinned buffers of `dtype` with at least `capacity` elements each: the cached ones while they still fit (pinning
        costs milliseconds; the loops view them per batch)."""
        ring = self._pinned.get(dtype)
        if ring is None or len(ring) != n or ring[0].numel() < capacity:
            ring = self._pinned[dtype] = [torch.zeros(capacity, dtype=dtype).pin_memory() for _ in range(n)]
        return ring

    def _pipeline(self, jobs, fill, take, lang_id, threshold, dtype=torch.float32, upload=None, graph=False):
        """The pipelined hot loop, for every encoder.  jobs[k] = (rows of forward k, values per staged row, frames per row): constant
        for Whisper (`batch_size` rows of `chunk_samples`, unused rows at lens 0), per batch for the by-length path.

        NS = `n_inflight` batches in flight on the GPU (two, or three for a BiLSTM behind a small encoder -- tagger.batches_in_flight;
        stream and workspace slot k % NS, own pinned output buffer), one more being filled: `fill(k, host[rows, values]) -> lens` (None:
        every row is full) runs on a worker thread one batch ahead of the launches (the native loader releases the GIL), into a ring of
        NS + 1 pinned input buffers of `dtype`, each guarded by the event of its last host-to-device copy; the main thread launches batch
        k and unpacks batch k - NS.  With everything on one thread (round 2's first half) the end-to-end rate of a folder of 30 s files
        was 82 k audio-s/s against 123 k for batches already resident.  The staging is flat pinned memory sized for the largest job and
        viewed per job (_pinned_ring).

        upload(host, lens, slot, stream) -> (device batch, lens): another staging format, run inside the slot's stream context (the GPU
        ingest path: int16 PCM rows, resampled on the device -- _label_resampled); default: float32 waveform rows copied as they are.
        graph: captured forwards (Whisper only), one slot, on the current stream.

        What callers rely on: `fill` of batch k + 1 runs while batch k is launched; `take(k, ids[rows, T], offsets[rows, T, 2])` is
        called in ascending k, after the forward's device-side status word (it rides behind the tags) went through raise_on_status,
        with views into pinned memory that are valid only until it returns: copy what you keep.

        (Two WavLM-base forwards in flight used to disturb each other now and then: a packed-f32 instruction form in the group-norm
        conv0 kernel that is unsafe beside another wave's MFMAs -- DESIGN.md section 7; the form is gone and the build refuses it;
        `test_two_wavlm_forwards_in_flight_do_not_disturb_each_other` guards the loop.)"""
        if not jobs:
            return
        NS = self.n_inflight
        NI = NS + 1
        pin_in = self._pinned_ring(NI, dtype, max(rows * width for rows, width, _ in jobs))
        pin_out = self._pinned_ring(NS, torch.int32, max(rows * T * 4 + 1 for rows, _, T in jobs))
        if self._streams is None or len(self._streams) != NS:
            self._streams = [torch.cuda.Stream(self.device) for _ in range(NS)]
        pending = [None] * NS
        copied = [None] * NI                               # event behind the last H2D copy out of input buffer i

        def staged(k):
            rows, width, _ = jobs[k]
            return pin_in[k % NI][:rows * width].view(rows, width)

        def fill_job(k):
            if copied[k % NI] is not None:
                copied[k % NI].synchronize()               # (NS + 1 batches back: long done)
            return fill(k, staged(k))

        def finish(slot):
            if pending[slot] is None:
                return
            k, ev = pending[slot]
            ev.synchronize()
            rows, _, T = jobs[k]
            nn = rows * T
            blob = pin_out[slot].numpy()
            raise_on_status(int(blob[4 * nn]))
            take(k, blob[0:nn].reshape(rows, T), blob[2 * nn:4 * nn].view(np.float32).reshape(rows, T, 2))
            pending[slot] = None

        with ThreadPoolExecutor(max_workers=1) as pool:
            fut = pool.submit(fill_job, 0)
            for k, (rows, _, T) in enumerate(jobs):
                lens = fut.result()
                if k + 1 < len(jobs):
                    fut = pool.submit(fill_job, k + 1)
                slot = 0 if graph else k % NS
                finish(slot)                               # the output buffer and workspace of this slot are free again
                stream = torch.cuda.current_stream(self.device) if graph else self._streams[slot]
                with torch.cuda.stream(stream):
                    if upload is None:
                        dev_wav = staged(k).to(self.device, non_blocking=True)
                    else:
                        dev_wav, lens = upload(staged(k), lens, slot, stream)
                    copied[k % NI] = torch.cuda.Event()
                    copied[k % NI].record(stream)
                    res = self.model.label(dev_wav, None if lang_id is None else [lang_id] * rows, threshold=threshold, lens=lens,
                                           average_languages=lang_id is None, graph=graph, slot=slot)
                    pin_out[slot][:rows * T * 4 + 1].copy_(res.packed, non_blocking=True)
                    ev = torch.cuda.Event()
                    ev.record(stream)
                pending[slot] = (k, ev)
            for k in range(max(0, len(jobs) - NS), len(jobs)):   # what is still in flight, oldest first
                finish(0 if graph else k % NS)

    def _forward_items_by_length(self, items, lang_id, threshold):
        """WavLM and the mel front-end: the frame count follows the clip length and the reference never pads their input (padding
        would change the waveform / GroupNorm statistics, the unmasked attention and where the backward LSTM starts).  A batch may
        still hold clips of different lengths: the library takes per-clip sample counts (`lens`) and carries every clip's own frame
        count through the whole forward, so each row comes out as if labelled alone (csrc/model.hip, Runner::clipT).  Clips are
        sorted by length so that a batch wastes little on its shorter rows; `WFL_RAGGED=0` goes back to one length per batch."""
        out = [None] * len(items)
        Bs = self.batch_size
        frames = [self.model.num_frames(len(x)) for x in items]
        for i, t in enumerate(frames):
            if t <= 0:
                raise ValueError(f"clip {i} is too short for the {self.model.encoder_type} front-end ({len(items[i])} samples)")
        if os.environ.get("WFL_RAGGED", "1") != "0":
            order = sorted(range(len(items)), key=lambda i: -len(items[i]))
            batches = [order[s:s + Bs] for s in range(0, len(order), Bs)]
        else:
            by_len = {}
            for i, x in enumerate(items):
                by_len.setdefault(len(x), []).append(i)
            batches = [idxs[s:s + Bs] for n, idxs in by_len.items() for s in range(0, len(idxs), Bs)]
        jobs = []
        for sel in batches:
            n = max(len(items[i]) for i in sel)
            jobs.append((len(sel), n, self.model.num_frames(n)))

        def fill(k, host):
            rows = host.numpy()
            lens = np.array([len(items[i]) for i in batches[k]], np.int32)
            for j, i in enumerate(batches[k]):
                rows[j, :lens[j]] = items[i]
                rows[j, lens[j]:] = 0.0                    # (behind a shorter clip: never read -- `lens` -- but keep the buffer defined)
            return None if (lens == host.shape[1]).all() else lens

        def take(k, ids, offs):
            for j, i in enumerate(batches[k]):
                out[i] = (ids[j, :frames[i]].copy(), offs[j, :frames[i]].copy())

        self._pipeline(jobs, fill, take, lang_id, threshold)
        return out

    def _lang_name(self, lang_id):
        if lang_id is None:
            return None
        for n, i in self.lang2id.items():
            if i == lang_id:
                return n
        return None

    def _names_for(self, lang_name):
        """phoneme index -> (index into unique output names, names): the merge-map back-mapping (utils.py:206-211) applied to
        the phoneme table once instead of to every segment; phonemes that map to the same string share an index, so the
        equal-neighbour merge compares exactly what the reference's string comparison compares."""
        key = lang_name if (self.merge_map and lang_name) else None
        cache = self._names_cache
        if key not in cache:
            mapped = [pp.canonical_to_lang(ph, key, self.merge_map) if key else ph for ph in self._table.names]
            uniq, remap = [], np.empty(max(len(mapped), 1), np.int32)
            index = {}
            for i, nm in enumerate(mapped):
                if nm not in index:
                    index[nm] = len(uniq)
                    uniq.append(nm)
                remap[i] = index[nm]
            cache[key] = (remap, uniq)
        return cache[key]

    def _segments_of_item(self, ids, offsets, lang_name):
        """suppressed ids -> median filter -> BIO decode -> merge-map back-mapping (infer.py:164-179, 293-307), in native
        code; returns (start[n] f64, end[n] f64, name index[n]) arrays."""
        mf = int(self.config["postprocess"]["median_filter"])
        s, e, ph = npost.decode_bio_ids(ids, self._table, frame_duration, offsets, median=mf)
        remap, _ = self._names_for(lang_name)
        return s, e, remap[ph] if ph.size else ph

    def _merged_tuples(self, s, e, ph, lang_name):
        """A file's segments (name indices of _names_for) -> merge_segments unless "none" -> [(start_s, end_s, phoneme)]."""
        mode = self.config["postprocess"]["merge_segments"]
        ph = ph.astype(np.int32)
        if mode != "none" and s.size:
            s, e, ph = npost.merge_segments(s, e, ph, mode)
        return npost.to_tuples(s, e, ph, self._names_for(lang_name)[1])

    def _file_segments(self, parts, lang_name):
        """A file's free decode: parts = [(ids, offsets, clock_s)] of its chunks in order (one for a file of at most 30 s) ->
        [(start_s, end_s, phoneme)] on the file's clock, merged and named."""
        if not parts:
            return self._merged_tuples(np.empty(0), np.empty(0), np.empty(0, np.int32), lang_name)
        segs = [self._segments_of_item(ids, offs, lang_name) for ids, offs, _ in parts]
        s, e = (np.concatenate([seg[c] + p[2] for seg, p in zip(segs, parts)]) for c in (0, 1))
        return self._merged_tuples(s, e, np.concatenate([seg[2] for seg in segs]), lang_name)

    def _label_rows(self, n_files, width, fill, lang_id, threshold, lang_name, dtype=torch.float32, upload=None):
        """One file per row of a Whisper batch, files k * batch_size ... in batch k: `fill(those file indices, host rows of `width`
        values) -> (lens for the pipeline, [(row, file index)] of the rows it accepted)`; a finished batch's accepted tags go to a
        second worker thread for the native median filter + BIO decode + segment merge while the next batches run.
        -> {file index: [(start_s, end_s, phoneme)]} (before forced alignment)."""
        Bs = self.batch_size
        meta, futures = {}, []
        self._names_for(lang_name)                       # (build the cache on this thread)
        post = ThreadPoolExecutor(max_workers=1)

        def fill_batch(k, host):
            lens, meta[k] = fill(list(range(k * Bs, min((k + 1) * Bs, n_files))), host)
            return lens

        def segments(rows):
            return [(fi, self._file_segments([(ids, offs, 0.0)], lang_name)) for fi, ids, offs in rows]

        def take(k, ids, offs):
            futures.append(post.submit(segments, [(fi, ids[r].copy(), offs[r].copy()) for r, fi in meta.pop(k)]))

        try:
            self._pipeline([(Bs, width, self.model.num_frames(self.chunk_samples))] * -(-n_files // Bs), fill_batch, take, lang_id,
                           threshold, dtype, upload, graph=self.use_graph)
            return {fi: seg for f in futures for fi, seg in f.result()}
        finally:
            post.shutdown(wait=True)

    def _label_fast(self, audio_paths, lang_id, threshold, lang_name):
        """Files the native loader takes whole (16 kHz, <= 30 s, <= 2 channels, PCM / float WAV): decoded, normalised and
        converted by worker threads straight into the pinned batch rows (audio.load_wavs_into), one file per row (_label_rows).
        Returns {file index: [(start_s, end_s, phoneme)]} (before forced alignment); every other file is left to the general path."""
        L = self.chunk_samples
        threads = _worker_threads()

        def fill(sel, host):
            ns, srs, st = A.load_wavs_into([audio_paths[i] for i in sel], host, L, threads)
            lens = np.zeros(self.batch_size, dtype=np.int32)
            ok = []
            for r, fi in enumerate(sel):
                if st[r] == 0 and srs[r] == self.sr and ns[r] > 0:
                    lens[r] = ns[r]
                    ok.append((r, fi))
            return lens, ok

        return self._label_rows(len(audio_paths), L, fill, lang_id, threshold, lang_name)

    def _label_resampled(self, audio_paths, src_sr, lang_id, threshold, lang_name):
        """Files of ONE sample rate other than the model's, 16-bit PCM, at most 30 s: their samples go to the GPU as they are (the native
        reader copies the file's PCM bytes into pinned int16 rows) and csrc/resample.hip decodes, resamples (float64 sinc, torchaudio's
        published algorithm: infer.py:217-220) and peak-normalises (infer.py:234-235) them into the batch the forward reads -- the host's
        cores no longer bound a 44.1 kHz folder (48 k audio-s/s with the host resampler).  Same pipeline, post-
        processing and result as _label_fast."""
        import ctypes as C

        from . import _lib
        lib = _lib.load()
        Bs, L = self.batch_size, self.chunk_samples
        cap_in = 2 * (int(math.ceil(L * src_sr / self.sr)) + 2)          # interleaved int16 values of a 30 s two-channel file
        ws_bytes = int(lib.wfl_resample_workspace_bytes(Bs, L))
        dev_out, dev_ws = {}, {}
        threads = _worker_threads()

        def fill(sel, host):
            nf, ch, srs, st = A.read_pcm16_into([audio_paths[i] for i in sel], host, cap_in, threads)
            frames = np.zeros(Bs, np.int32)
            chans = np.ones(Bs, np.int32)
            ok = []
            for r, fi in enumerate(sel):
                if st[r] == 0 and srs[r] == src_sr and nf[r] > 0 and int(math.ceil(int(nf[r]) * self.sr / src_sr)) <= L:
                    frames[r], chans[r] = nf[r], ch[r]
                    ok.append((r, fi))
            return (frames, chans), ok

        def upload(host, fc, slot, stream):
            frames, chans = fc
            if slot not in dev_out:
                dev_out[slot] = torch.zeros(Bs, L, dtype=torch.float32, device=self.device)
                dev_ws[slot] = torch.empty(ws_bytes, dtype=torch.uint8, device=self.device)
            d_pcm = host.to(self.device, non_blocking=True)
            d_meta = torch.from_numpy(np.stack([frames, chans])).to(self.device)
            rc = lib.wfl_resample_pcm16(C.c_void_p(d_pcm.data_ptr()), cap_in, C.c_void_p(d_meta[0].data_ptr()), C.c_void_p(d_meta[1].data_ptr()),
                                        Bs, int(src_sr), int(self.sr), C.c_void_p(dev_out[slot].data_ptr()), L, L,
                                        C.c_void_p(dev_ws[slot].data_ptr()), ws_bytes, C.c_void_p(stream.cuda_stream))
            _lib.check(rc, "wfl_resample_pcm16")
            d_pcm.record_stream(stream)
            d_meta.record_stream(stream)
            lens = np.minimum(np.ceil(frames.astype(np.float64) * self.sr / src_sr), L).astype(np.int32)
            return dev_out[slot], lens

        return self._label_rows(len(audio_paths), cap_in, fill, lang_id, threshold, lang_name, torch.int16, upload)

    def options(self, **given) -> PostOptions:
        """The post-processing options of a request (options.resolve): an argument that is given wins, the others come from this
        Labeler's config `postprocess` section, else the defaults; ValueError for a request the rules between them refuse."""
        return resolve(self.config.get("postprocess"), **given)

    def _bigram_table(self, path, switch_penalty, weight):
        """The search's transition table for the bigram file `path` (absolute, or relative to the working directory)."""
        from . import phonotactics as PH
        key = (os.path.abspath(path), float(switch_penalty), float(weight))
        if key not in self._bigram_cache:
            if self._decode_table is None:
                self._decode_table = DC.class_table(self.labels)
            self._bigram_cache[key] = PH.transition_table(PH.load(key[0]), self._decode_table, self.labels, switch_penalty, weight)
        return self._bigram_cache[key]

    def _duration_prior(self, path, weight, lang_name):
        """-> (durations.DurationPrior, its float32 table at `weight`) of the file `path` (absolute, or relative to the working
        directory), checked against the frame clock and the label set's output names."""
        from . import durations as DU
        key = ("durations", os.path.abspath(path), float(weight), lang_name)
        if key not in self._bigram_cache:
            prior = DU.load(key[1])
            DU.check(prior, self._names_for(lang_name)[1], frame_duration, path=str(path))
            self._bigram_cache[key] = (prior, DU.table(prior, weight))
        return self._bigram_cache[key]

    def _decode_duration_prior(self, path, weight, switch_penalty, trans, lang_name):
        """The free decode's duration prior (opts.decode_duration_prior) -> (trans, dur, sym_dur) for decode.bio_viterbi_duration (a label
        set over the search's symbol cap is reported by the search, status 2, as the bigram's is).  trans: the phoneme
        bigram's table, or None: the flat table -switch_penalty, wfl_decode's objective.  The prior is _duration_prior's (loaded, checked
        against the frame clock and the output names, scaled by `weight`); a phoneme's row is the one of its output name."""
        prior, dur = self._duration_prior(path, weight, lang_name)
        if self._decode_table is None:
            self._decode_table = DC.class_table(self.labels)
        table = self._decode_table
        n = len(table[1]) + 1
        if trans is None:
            trans = np.full((n, n), -float(switch_penalty), np.float32)
        remap, names = self._names_for(lang_name)
        out = {ph: names[int(remap[i])] for i, ph in enumerate(self._table.names)}
        return trans, dur, DC.duration_symbol_rows(prior, table, self.labels, out)

    def label_files(self, audio_paths, lang_id=None, confidence_threshold=0.0, verbose=True, align=None, align_scores=None,
                    decode=None, switch_penalty=None, decode_scores=None, phoneme_bigram=None, bigram_weight=None, align_draft=None,
                    draft_tolerance=None, align_edits=None, align_insertions=None, min_duration=None, duration_scores=None,
                    optional_tokens=None, skip_penalty=None, optional_scores=None, filler_token=None, filler_penalty=None,
                    filler_scores=None, duration_prior=None, duration_prior_weight=None, duration_prior_scores=None,
                    decode_duration_prior=None, decode_duration_prior_weight=None, decode_duration_scores=None,
                    transcript_variants=None, bigram_scores=None):
        """-> list (per file) of [(start_s, end_s, phoneme)] after merge + forced alignment; with align_scores, duration_scores,
        decode_scores, bigram_scores or decode_duration_scores, (that list, scores); with align_edits the tuple goes on with one more list, edits, and with
        align_insertions it ends with one more, insertions; with optional_tokens it ends with the list skipped; with a filler_token
        it ends with the list fillers, and with filler_scores with one more, filler_scores; with duration_prior_scores it ends with the
        list durations.

        align: "greedy" -- a `{audio}.txt` transcript is matched onto the freely decoded segments (infer.py:30-60, 312-319);
        "viterbi" -- files with a transcript are aligned by a search over their frame logits on the GPU (align.py: one segment
        per token, in order, none dropped); files without one take the greedy path unchanged.  None: config postprocess.align.

        align_scores (with "viterbi" only; None: config postprocess.align_scores, else off): also return scores[i], an
        align.FileScore from a forward-backward pass over the file's alignment lattice (per token the posterior of the run it got
        and the spread of its start), or None for a file without a transcript or one that fell back to the greedy alignment (and,
        with a message, for an aligned file whose path wfl_align_posterior does not accept: status 8, not expected from wfl_align's
        own output).  The segments are the same with and without.

        decode: "argmax" -- the free decode is the reference's (per-frame argmax, confidence threshold, median filter, BIO decoder);
        "viterbi" -- every file whose segments come from the free decode (no transcript, or one under align "greedy", which is then
        matched over the new segments) is decoded by the BIO-grammar search over its frame logits on the GPU (decode.py), each opened
        run costing `switch_penalty` nats; postprocess.median_filter is not applied to those files.  None: config postprocess.decode /
        postprocess.switch_penalty, else argmax / 0.

        phoneme_bigram (with decode "viterbi" only; None: config postprocess.phoneme_bigram, else none): a phoneme_bigram.json
        (phonotactics.py); the search then pays  bigram_weight * log P(opened symbol | previous symbol) - switch_penalty  for every
        opened run instead of the flat penalty (decode.bio_viterbi_bigram).  bigram_weight: a number >= 0 (None: config
        postprocess.bigram_weight, else 1).  decode_scores cannot be combined with a bigram; bigram_scores is its counterpart there.

        decode_scores (with decode "viterbi" only; None: config postprocess.decode_scores, else off): also return scores[i], a
        decode.FreeScore from a forward-backward pass over the grammar for a file the grammar search decoded (per run of the path, before
        merge_segments and any string match, the posterior of its phoneme, of its opening frame and of its weakest frame), or None for a
        file that fell back to the argmax decode (and, with a message, for one whose path wfl_decode_posterior does not accept).  With
        both kinds of scores on, each file gets its own kind.  The segments are the same with and without.

        bigram_scores (with a phoneme_bigram only; None: config postprocess.bigram_scores, else off): decode_scores for a bigram
        decode -- the same scores[i] records, from a forward-backward pass over the grammar with the bigram's transition table
        (decode.decode_posteriors_bigram), so the posterior scores the grammar the search ran on.  The segments are the same with and
        without.

        align_draft (with align "viterbi" only; None: config postprocess.align_draft, else none): a folder of draft .lab files, the
        draft of X.wav being DIR/X.lab.  A file with a draft is aligned to the draft's label sequence (SP / AP included as tokens, as
        when a .txt spells them; it wins over a .txt that spells something else, with a message), every token opening within
        draft_tolerance seconds (>= 0; None: config postprocess.draft_tolerance, else 0.1) of its draft start: the windowed search
        of align.viterbi_align, and with align_scores the windowed forward-backward over the same lattice.  A draft whose windows no
        path satisfies (align.windows_feasible) falls back, with a message, to the unwindowed search of the same transcript.  Files
        without a draft are handled as without the option.

        align_edits (with align "viterbi" only; None: config postprocess.align_edits, else off): also return edits[i], for a file
        that was Viterbi-aligned one align.TokenEdit per transcript token -- the best and the second-best substitute phoneme with the
        log likelihood ratio of the transcript so edited against the transcript as written, the same for the transcript without the
        token, and a flag where the largest is > 0 (align.edit_scores: sums over all boundaries of the lattice the search ran on, the
        draft's windows included) -- or None for a file without a transcript or one that fell back to the greedy alignment (with a
        message).  The segments are the same with and without.

        align_insertions (with align "viterbi" only; None: config postprocess.align_insertions, else off): also return
        insertions[i], for a file that was Viterbi-aligned one align.PlaceInsertion per place of the transcript (in front of every
        token, and behind the last) -- the best and the second-best phoneme to insert there with the log likelihood ratio of the
        longer transcript against the transcript as written, and a flag where the best is > 0 (align.insertion_scores: on the same
        lattice as the edits, the inserted token without a window) -- or None as for align_edits.  The segments and the edits are
        the same with and without.

        min_duration (with align "viterbi" only; None: config postprocess.min_duration, else none): seconds, or a mapping {token
        name: seconds, "default": seconds} -- the least time every transcript token (the named ones) occupies, held by the search
        itself (align.viterbi_align's min_frames, align.min_frames_for: at most 8 frames).  Only transcript tokens are constrained,
        not the SP / AP of gaps, not the free decode.  It combines with align_draft; align_scores, align_edits and
        align_insertions beside it are refused (their passes score the lattice without durations).  A file whose durations no path
        can meet falls back, with a message, to the alignment of the same transcript without them (the draft's windows kept).

        duration_scores (with a min_duration only; None: config postprocess.duration_scores, else off): align_scores for an
        alignment under minimum durations -- the same scores[i] (align.FileScore), from align.duration_posteriors over the
        minimum-duration lattice of the search, on the PackedClips it ran on.  A file whose durations were dropped is scored by
        align.alignment_posteriors, over the lattice without them it was searched on, and one line says so.

        optional_tokens (with align "viterbi" only; None: config postprocess.optional_tokens, else none): a list of token names
        (output names, as a transcript spells them), or "*" for every token -- the transcript tokens a path may leave out, at most
        one between two kept ones (align.viterbi_align_optional), each at skip_penalty nats (>= 0; None: config
        postprocess.skip_penalty, else 0).  The segments of such a file lack the skipped tokens, one line says how many, and
        skipped[i] is one align.SkippedToken per token left out (None for a file that was not aligned that way).  It combines with
        align_draft (the names are the draft's labels; kept tokens hold their windows); min_duration and the scoring options beside
        it are refused.  A name that is no output name of the label set is refused by name.
        optional_scores (with optional_tokens only; None: config postprocess.optional_scores, else off): align_scores for that
        search, summed over its skip lattice (align.optional_posteriors): scores[i] is an align.FileScore over the kept tokens, and
        the result ends with one more list, optional: per file one align.OptionalTokenScore per optional token of its transcript --
        kept or skipped, the posterior probability that the token is present, and `doubt` where the other decision has more
        posterior mass (None for a file that was not scored that way).

        filler_token (with align "viterbi" only; None: config postprocess.filler_token, else none): a name; a transcript token equal
        to it is a filler, a token like any other (one contiguous run of at least one frame, in order, gaps possible on both sides)
        that matches anything: every frame of its run scores the frame's largest logit over all classes minus filler_penalty nats
        (>= 0; None: config postprocess.filler_penalty, else 1.0 -- a value to start from, not a measured optimum), so a frame goes to
        the filler instead of a neighbouring token only where that token's class is more than the penalty below the frame's best
        class (align.viterbi_align_filler).  Runs of adjacent fillers are collapsed into one, with a line.  In the segments a
        filler's span holds what the file's own free decode found there (align.filler_segments), and fillers[i] is one
        align.FillerSpan per filler (None for a file that was not aligned that way).  The greedy match a file falls back to gets
        the transcript without its fillers.  A filler_token that is an output name of the label set is refused by name; align_draft,
        min_duration, optional_tokens and the scoring options beside it are refused.

        filler_scores (with a filler_token only; None: config postprocess.filler_scores, else off): scores[i] is the align.FileScore
        of a file that was aligned, from a forward-backward pass over the lattice the file was searched on -- the filler lattice
        (align.filler_posteriors, the same flags and penalty) for a file with a filler, wfl_align_posterior's for one without, with
        one line -- and filler_scores[i] one align.FillerScore per filler: the posterior that its span's frames belong to it and the
        mean shift and spread of both its ends (None for a file that was not aligned or not scored).

        duration_prior (with align "viterbi" only; None: config postprocess.duration_prior, else none): a phoneme_durations.json
        (python -m wfl_asr_amd.durations): a file with a transcript is aligned by the explicit-duration search
        (align.viterbi_align_duration_prior), in which a run of d frames of a token adds duration_prior_weight (>= 0; None: config
        postprocess.duration_prior_weight, else 1.0 -- a value to start from, not a measured optimum) times the log probability the
        prior gives d frames of that phoneme; the row is the one of the token's output name as the transcript spells it, a token the
        prior does not hold has none.  A file the prior leaves no path for falls back, with a line, to the plain alignment of the same
        transcript.  A prior counted on another frame duration, or one that holds a phoneme that is no output name of the label set,
        is refused by name; align_draft, min_duration, optional_tokens, filler_token and the scoring options beside it are refused.

        duration_prior_scores (with a duration_prior only; None: config postprocess.duration_prior_scores, else off): scores[i] is the
        align.FileScore of a file that was aligned, from a forward-backward pass over the lattice the file was searched on -- the
        explicit-duration lattice (align.duration_prior_posteriors, the rows, the table and the weight of the search) for a file
        searched under the prior, wfl_align_posterior's, with one line, for one the prior left no path for -- and durations[i] one
        align.TokenDuration per transcript token of a file scored under the prior: its run, the prior's log probability of that
        length, the posterior of the run, the mean shift and spread of both its ends and the expected length (None for a file that
        was not aligned, or was searched without the prior).  The segments are the same with and without.

        decode_duration_prior (with decode "viterbi" only; None: config postprocess.decode_duration_prior, else none): a
        phoneme_durations.json for the FREE decode: every file the grammar search decodes is searched by the explicit-duration search
        (decode.bio_viterbi_duration, wfl_decode_duration), in which a run of d frames of a phoneme adds decode_duration_prior_weight
        (>= 0; None: config postprocess.decode_duration_prior_weight, else 1.0 -- a value to start from, not a measured optimum)
        times the log probability the prior gives d frames of the phoneme's output name; a phoneme the prior does not hold has none, and
        O runs carry none.  Opened runs cost what they cost without the prior: the phoneme_bigram's table where one is given, else the
        flat switch penalty.  A file's chunks are one clip, so a run that crosses a chunk seam is one run and pays one prior.  The
        file is checked as a duration_prior is; decode_scores and bigram_scores beside it are refused: decode_duration_scores is their
        counterpart there.  `duration_prior` keeps meaning the transcript alignment's prior.

        decode_duration_scores (with a decode_duration_prior only; None: config postprocess.decode_duration_scores, else off):
        decode_scores for a duration-prior decode -- the same scores[i] records, from a semi-Markov forward-backward pass over the
        grammar with the search's transition table and duration table (decode.decode_posteriors_duration,
        wfl_decode_duration_posterior), so the posterior scores the grammar the search ran on.  The segments are the same with and
        without.

        transcript_variants (with align "viterbi" only; None: config postprocess.transcript_variants, else off): `(`, `|` and `)` in
        a `{audio}.txt` are syntax -- `k a ( t | d ) o ( N | ) ( ts u | s u )` offers 2 to 4 spellings of a stretch, the first the
        transcript as written, an empty one making the stretch optional -- and a file whose transcript holds such a group is
        searched over the graph of all of them (align.viterbi_align_graph, wfl_align_graph): the variants are chosen jointly.  Its
        segments are the chosen slots'; the tuple ends with the list variants, per such file its align.VariantChoice rows.  A file
        without a group is searched by exactly the calls it is searched by without the option.  The greedy fallback and the
        end-pause rule take the transcript as written.  A malformed transcript is refused, naming the file and the place; the
        options whose lattices are chains are refused beside it, each by name."""
        opts = self.options(align=align, align_scores=align_scores, decode=decode, switch_penalty=switch_penalty,
                            decode_scores=decode_scores, phoneme_bigram=phoneme_bigram, bigram_weight=bigram_weight,
                            bigram_scores=bigram_scores, align_draft=align_draft, draft_tolerance=draft_tolerance,
                            align_edits=align_edits, align_insertions=align_insertions, min_duration=min_duration,
                            duration_scores=duration_scores, optional_tokens=optional_tokens, skip_penalty=skip_penalty,
                            optional_scores=optional_scores, filler_token=filler_token, filler_penalty=filler_penalty,
                            filler_scores=filler_scores, duration_prior=duration_prior, duration_prior_weight=duration_prior_weight,
                            duration_prior_scores=duration_prior_scores, decode_duration_prior=decode_duration_prior,
                            decode_duration_prior_weight=decode_duration_prior_weight, decode_duration_scores=decode_duration_scores,
                            transcript_variants=transcript_variants)
        reports = R.Reports.for_options(opts)
        final, scores = self._label_scored(audio_paths, opts, lang_id, confidence_threshold, verbose, reports)
        out = (final, scores) if opts.scored else (final,)
        for by_file in reports.rows.values():             # (the enabled kinds, in reports.REPORTS' order)
            out += ([by_file.get(fi) for fi in range(len(audio_paths))],)
        return out if len(out) > 1 else final

    def _label_scored(self, audio_paths, opts, lang_id, confidence_threshold, verbose, reports=None):
        """label_files for the resolved options `opts`, always -> (segments, scores): the files are split once into those a transcript is
        Viterbi-aligned to, those the grammar search decodes and those left to the argmax decode, and each subset's results go back to
        its files' places.  reports (reports.Reports.for_options(opts); None: nothing is kept): takes the draft moves and, per enabled
        kind of side report, the rows of every file that was Viterbi-aligned that way, by file index."""
        if filler_token_collision(opts.filler_token, self._names_for(self._lang_name(lang_id))[1]) is not None:
            raise ValueError(f"filler_token: {opts.filler_token!r} is an output name of this model's label set")
        unknown = (unknown_optional_tokens(opts.optional_tokens, self._names_for(self._lang_name(lang_id))[1])
                   if opts.optional_tokens not in (None, "*") else [])
        if unknown:
            raise ValueError(f"optional_tokens: {', '.join(repr(n) for n in unknown)} is no output name of this model's label set")
        trans = self._bigram_table(opts.phoneme_bigram, opts.switch_penalty, opts.bigram_weight) if opts.phoneme_bigram else None
        prior = (self._duration_prior(opts.duration_prior, opts.duration_prior_weight, self._lang_name(lang_id))
                 if opts.duration_prior else None)
        free_prior = (self._decode_duration_prior(opts.decode_duration_prior, opts.decode_duration_prior_weight, opts.switch_penalty,
                                                  trans, self._lang_name(lang_id)) if opts.decode_duration_prior else None)
        if opts.decode == "viterbi" and int(self.config["postprocess"].get("median_filter", 0)) > 1:
            print("decode: viterbi -- postprocess.median_filter is not applied (the switch penalty takes its place)")
        if lang_id is not None and self.lang2id and lang_id > max(self.lang2id.values()):
            raise ValueError(f"Error: Language ID ({lang_id}) is higher than the latest ID ({max(self.lang2id.values())}) "
                             f"of this model.\n Languages and Codes available: {self.lang2id}")
        final, scores = [None] * len(audio_paths), [None] * len(audio_paths)
        free, with_t, graphs = list(range(len(audio_paths))), [], {}
        if opts.align == "viterbi":
            forced = [_read_forced(p, verbose) for p in audio_paths]
            drafts = [_read_draft(p, opts.align_draft, forced[fi]) if opts.align_draft else None for fi, p in enumerate(audio_paths)]
            forced = [tr if dr is None else [s[2] for s in dr] for tr, dr in zip(forced, drafts)]
            if opts.filler_token is not None:             # runs of adjacent fillers are one filler
                for fi, tr in enumerate(forced):
                    if tr:
                        forced[fi], merged = AL.collapse_fillers(tr, opts.filler_token)
                        if merged:
                            print(f"{audio_paths[fi]}: {merged} adjacent filler tokens collapsed")
            if opts.transcript_variants:                  # a transcript with groups: its graph; the file goes on as written
                graphs = _read_variants(audio_paths, forced, self._names_for(self._lang_name(lang_id))[1])
            with_t = [fi for fi in free if forced[fi] is not None]
            free = [fi for fi in free if forced[fi] is None]

        def paths(idx):
            return [audio_paths[fi] for fi in idx]

        searched = {}
        if opts.decode == "viterbi":
            # the free decode by the grammar search; a file it could not decode (with a message) takes the argmax decode
            got, free_scores = self._decode_viterbi(paths(free), lang_id, confidence_threshold, verbose, opts.switch_penalty,
                                                    opts.free_scores, trans, free_prior)
            searched = {free[j]: segs for j, segs in got.items()}
            for j, sc in free_scores.items():
                scores[free[j]] = sc
        argmax = [fi for fi in free if fi not in searched]
        for fi, segs in zip(argmax, self._label_files_greedy(paths(argmax), lang_id, confidence_threshold, verbose)):
            final[fi] = segs
        for fi, segs in searched.items():
            final[fi] = self._match_forced(audio_paths[fi], segs, verbose)
        if with_t:
            got = self._label_viterbi(paths(with_t), [forced[fi] for fi in with_t], [drafts[fi] for fi in with_t], opts, lang_id,
                                      confidence_threshold, verbose, prior,
                                      **({"graphs": {j: graphs[fi] for j, fi in enumerate(with_t) if fi in graphs}} if graphs else {}))
            for fi, rec in zip(with_t, got):
                final[fi], scores[fi] = rec.segments, rec.score
                if reports is not None:
                    reports.take(fi, rec.rows, rec.moves)
        return final, scores

    def _label_files_greedy(self, audio_paths, lang_id, confidence_threshold, verbose):
        """The argmax free decode of every file, then the greedy match of its transcript, if it has one (_match_forced)."""
        lang_name = self._lang_name(lang_id)
        decided_fast = {}                                 # file index -> segments of its one <= 30 s item, natively loaded
        if self.model.encoder_type == "whisper" and len(audio_paths) > 0:
            # only files whose header says 16 kHz are offered to the fast path (the others would be decoded there just to be turned
            # away, and their rows forwarded empty); a header that cannot be read leaves the decision to the loader
            cand = [fi for fi, p in enumerate(audio_paths) if A.wav_sample_rate(p) in (self.sr, None)]
            if cand:
                got = self._label_fast([audio_paths[fi] for fi in cand], lang_id, confidence_threshold, lang_name)
                decided_fast = {cand[j]: seg for j, seg in got.items()}
            # files at another rate: 16-bit PCM of at most 30 s goes to the GPU as it is and is resampled there (WFL_GPU_INGEST=0: host)
            if os.environ.get("WFL_GPU_INGEST", "1") != "0":
                by_rate = {}
                for fi, p in enumerate(audio_paths):
                    if fi in decided_fast:
                        continue
                    h = A.wav_header(p)
                    if h is None:
                        continue
                    tag, ch, sr, bits, nbytes = h
                    if tag == 1 and bits == 16 and ch in (1, 2) and sr != self.sr and sr > 0:
                        frames = nbytes // (2 * ch)
                        if 0 < frames and int(math.ceil(frames * self.sr / sr)) <= self.chunk_samples:
                            by_rate.setdefault(sr, []).append(fi)
                for sr, fis in by_rate.items():
                    got = self._label_resampled([audio_paths[fi] for fi in fis], sr, lang_id, confidence_threshold, lang_name)
                    decided_fast.update({fis[j]: seg for j, seg in got.items()})
        items, owner, clocks = [], [], []
        clock = [0.0] * len(audio_paths)
        load_one = self._load_chunks

        slow = [fi for fi in range(len(audio_paths)) if fi not in decided_fast]
        # The native loader releases the GIL: files decode / resample on worker threads, all submitted at once; the items are
        # forwarded in waves, in file order, as their files arrive, so the forwards of one wave run under the loading of the next.
        decided = []
        pool = None
        try:
            if len(slow) > 1:
                pool = ThreadPoolExecutor(max_workers=_worker_threads(len(slow)))
                futs = [pool.submit(load_one, audio_paths[fi]) for fi in slow]
            wave = self._wave()                           # items per wave: enough batches to fill the pipeline's slots
            start = 0
            for j, fi in enumerate(slow):
                chunks = futs[j].result() if pool is not None else load_one(audio_paths[fi])
                if verbose and len(chunks) > 1:
                    print(f"Audio is too long ({sum(len(c) for c in chunks)/self.sr:.1f}s), splitting...")
                for c in chunks:
                    items.append(c)
                    owner.append(fi)
                    clocks.append(clock[fi])
                    clock[fi] += len(c) / self.sr
                if len(items) - start >= wave and j + 1 < len(slow):
                    decided.extend(self._forward_items(items[start:], lang_id, confidence_threshold))
                    start = len(items)
            if len(items) > start:
                decided.extend(self._forward_items(items[start:], lang_id, confidence_threshold))
        finally:
            if pool is not None:
                pool.shutdown(wait=True, cancel_futures=True)
        parts = [[] for _ in audio_paths]
        for (ids, offs), fi, t0 in zip(decided, owner, clocks):
            parts[fi].append((ids, offs, t0))
        # (a file of decided_fast: one <= 30 s item, decoded and merged by the post worker already)
        return [self._match_forced(path, decided_fast[fi] if fi in decided_fast else self._file_segments(parts[fi], lang_name), verbose)
                for fi, path in enumerate(audio_paths)]

    @staticmethod
    def _match_forced(path, segs, verbose):
        """The greedy string match of a `{audio}.txt` transcript onto freely decoded segments and the pause rule for the ends
        (infer.py:30-60, 312-319); a file without a transcript keeps its segments."""
        forced = _read_forced(path, verbose)
        if forced is None:
            return segs
        return AL.with_end_pauses(segs, pp.align_phoneme_list(segs, forced), forced)

    def _wave(self):
        """Chunks per wave of files: enough batches to fill the pipeline's slots (a test sets a small `_wave_items`)."""
        return self._wave_items or max(8 * self.batch_size, 64)

    def _load_chunks(self, path):
        chunks = A.load_items(path, self.sr)            # native: decode, resample, normalise, 30 s chunks (csrc/hostpost.hip)
        if chunks is None:                              # an encoding the native decoder does not take: the Python restatement
            audio = A.load_clip(path, self.sr)
            chunks = A.chunk_clip(audio, self.sr)
        return chunks

    def _valid_frames(self, n, T):
        """Frames of a chunk of n samples in a forward of T frames: Whisper's window always has T frames, of which
        ceil(n T / chunk_samples) hold audio (min(1500, ceil(n / 320)) at 16 kHz); WavLM and the mel front-end: num_frames(n)."""
        if self.model.encoder_type == "whisper":
            return min(T, -(-n * T // self.chunk_samples))
        return self.model.num_frames(n)

    def _forward_with_logits(self, sel, by_file, lang_id, threshold):
        """Forward the chunks of a wave of files (by_file[fi]: the file's chunks) with the logits kept on the device ->
        (free, rows): (file, chunk) -> (ids, offsets) of the argmax decode as _forward_items returns them, and
        (file, chunk) -> (device logits rows of the chunk's valid frames, their offsets)."""
        Bs = self.batch_size
        whisper = self.model.encoder_type == "whisper"
        free, rows = {}, {}
        order = [(fi, ci) for fi in sel for ci in range(len(by_file[fi]))]
        if not whisper:
            order.sort(key=lambda k: -len(by_file[k[0]][k[1]]))
        for s0 in range(0, len(order), Bs):
            part = order[s0:s0 + Bs]
            xs = [by_file[fi][ci] for fi, ci in part]
            L = self.chunk_samples if whisper else max(len(x) for x in xs)
            host = np.zeros((len(xs) if not whisper else Bs, L), np.float32)
            lens = np.zeros(host.shape[0], np.int32)
            for r, x in enumerate(xs):
                n = min(len(x), L)
                host[r, :n] = x[:n]
                lens[r] = n
            same = (not whisper) and all(len(x) == L for x in xs)
            res = self.model.label(torch.from_numpy(host).to(self.device), None if lang_id is None else [lang_id] * host.shape[0],
                                   threshold=threshold, lens=None if same else lens, average_languages=lang_id is None,
                                   want_logits=True)
            raise_on_status(int(res.status.item()))
            T = res.ids.shape[1]
            ids_h, offs_h = res.ids.cpu().numpy(), res.offsets.cpu().numpy()
            for r, (fi, ci) in enumerate(part):
                tv = self._valid_frames(len(xs[r]), T)
                keep = T if whisper else tv                # what the greedy loop decodes (_forward_items)
                free[(fi, ci)] = (ids_h[r, :keep].copy(), offs_h[r, :keep].copy())
                rows[(fi, ci)] = (res.logits[r, :tv], offs_h[r, :tv].copy())
        return free, rows

    def _file_waves(self, audio_paths, verbose):
        """The files of a whole-file search (_decode_viterbi, _label_viterbi) in waves whose chunks are forwarded together: yields
        (files, by_file), the wave's file indices in order and {file: its chunks} for those that hold audio.  A pool loads the files
        ahead; a wave closes once it holds `wave` chunks."""
        if not audio_paths:
            return
        wave = self._wave()
        pool = ThreadPoolExecutor(max_workers=_worker_threads(len(audio_paths)))
        loads = [pool.submit(self._load_chunks, p) for p in audio_paths]      # (the native loader releases the GIL)
        pool.shutdown(wait=False)
        files = list(range(len(audio_paths)))
        while files:
            sel, by_file, n_chunks = [], {}, 0
            while files and n_chunks < wave:
                fi = files.pop(0)
                cs = loads[fi].result()
                loads[fi] = None
                if verbose and len(cs) > 1:
                    print(f"Audio is too long ({sum(len(c) for c in cs)/self.sr:.1f}s), splitting...")
                sel.append(fi)
                if cs:
                    by_file[fi] = list(cs)
                n_chunks += len(cs)
            yield sel, by_file

    @staticmethod
    def _file_rows(rows, by_file, sel):
        """-> (frames per file of `sel`, those files' valid logits rows concatenated on the device): one clip per file."""
        frames = [sum(rows[(fi, ci)][0].shape[0] for ci in range(len(by_file[fi]))) for fi in sel]
        return frames, torch.cat([rows[(fi, ci)][0] for fi in sel for ci in range(len(by_file[fi]))])       # device-to-device

    def _chunk_plan(self, rows, chunks, fi):
        """-> (chunk_frames, chunk_offsets, chunk_clock) of file fi for path_segments / path_segments_free."""
        cf, co, cc, clock = [], [], [], 0.0
        for ci, x in enumerate(chunks):
            r, offs = rows[(fi, ci)]
            cf.append(r.shape[0])
            co.append(offs)
            cc.append(clock)
            clock += len(x) / self.sr
        return cf, co, cc

    def _decode_viterbi(self, audio_paths, lang_id, threshold, verbose, switch_penalty, want_scores=False, trans=None, free_prior=None):
        """decode="viterbi": the free decode of files by the BIO-grammar search (decode.py, wfl_decode) -> ({file index: segments
        [(start_s, end_s, phoneme)] after the merge-map names and merge_segments, before any string match}, {file index: FreeScore}).  The files' chunks are
        forwarded with logits (kept on the device); each file's chunks' valid logits rows are concatenated on the device, so one
        search covers the whole file and a run may cross a chunk seam; the files of a wave go to wfl_decode as one ragged batch and
        only ids / status come back to the host.  A file whose status is not 0 is left out (with a message): the caller decodes it
        by argmax.  want_scores: right after the search, one wfl_decode_posterior call per wave over the clips it decoded (same
        logits, the device `ids`; wfl_decode_bigram_posterior with the same table when the search was the bigram's,
        wfl_decode_duration_posterior with the same tables when it was the duration prior's) and one log-sum-exp reduction over the wave's logits, the per-frame arrays back in one more copy; without, the second dict stays empty and the calls are
        the search's alone.  trans: the transition table of a phoneme bigram (_bigram_table); the search is then wfl_decode_bigram's,
        everything around it the same.  free_prior: _decode_duration_prior's triple; the search is then wfl_decode_duration's under its
        tables."""
        lang_name = self._lang_name(lang_id)
        remap, names = self._names_for(lang_name)
        if self._decode_table is None:
            self._decode_table = DC.class_table(self.labels)
        table = self._decode_table
        out, scored = {}, {}
        for files, by_file in self._file_waves(audio_paths, verbose):
            sel = [fi for fi in files if fi in by_file]
            out.update((fi, []) for fi in files if fi not in by_file)      # no audio: no segments
            if not sel:
                continue
            _, rows = self._forward_with_logits(sel, by_file, lang_id, threshold)
            frames, lg = self._file_rows(rows, by_file, sel)
            if free_prior is not None:
                d_ids, d_score, d_st = DC.bio_viterbi_duration(lg, frames, table, *free_prior, threshold)
            elif trans is None:
                d_ids, d_score, d_st = DC.bio_viterbi(lg, frames, table, switch_penalty, threshold)
            else:
                d_ids, d_score, d_st = DC.bio_viterbi_bigram(lg, frames, table, trans, threshold)
            ids_all, st_all = d_ids.cpu().numpy(), d_st.cpu().numpy()
            f0 = back_to_back(frames)
            raw = {}                                          # clip -> (score, logz, sum lse, post, cls_post, posterior status)
            ok = [b for b in range(len(sel)) if st_all[b] == DC.STATUS_OK]
            if want_scores and ok:
                if free_prior is not None:
                    d_logz, d_post, d_cls, d_pst = DC.decode_posteriors_duration(lg, [frames[b] for b in ok], table, *free_prior, threshold,
                                                                                 d_ids, frame_offsets=f0[ok])
                elif trans is None:
                    d_logz, d_post, d_cls, d_pst = DC.decode_posteriors(lg, [frames[b] for b in ok], table, switch_penalty, threshold,
                                                                        d_ids, frame_offsets=f0[ok])
                else:
                    d_logz, d_post, d_cls, d_pst = DC.decode_posteriors_bigram(lg, [frames[b] for b in ok], table, trans, threshold,
                                                                               d_ids, frame_offsets=f0[ok])
                d_lse = _clip_lse(lg, f0[ok], f0[ok] + np.asarray(frames, np.int64)[ok])
                n_ok, nr = len(ok), lg.shape[0]
                h = torch.cat([d_score[ok].double(), d_logz.double(), d_lse, d_pst.double(), d_post.double(), d_cls.double()]).cpu().numpy()
                for j, b in enumerate(ok):                    # one copy
                    a, z = int(f0[b]), int(f0[b]) + frames[b]
                    raw[b] = (h[j], h[n_ok + j], h[2 * n_ok + j], h[4 * n_ok + a:4 * n_ok + z], h[4 * n_ok + nr + a:4 * n_ok + nr + z],
                              int(h[3 * n_ok + j]))
            pos = 0
            for b, fi in enumerate(sel):
                n = frames[b]
                if st_all[b] != DC.STATUS_OK:
                    fn = "wfl_decode_duration" if free_prior is not None else ("wfl_decode" if trans is None else "wfl_decode_bigram")
                    print(f"{audio_paths[fi]}: viterbi decode not possible ({fn} status {int(st_all[b])}); using the argmax decode")
                else:
                    plan = self._chunk_plan(rows, by_file[fi], fi)
                    s, e, ph = DC.path_segments_free(ids_all[pos:pos + n], *plan, self._table, frame_duration)
                    out[fi] = self._merged_tuples(s, e, remap[ph] if ph.size else ph, lang_name)
                    if b in raw and raw[b][5] == DC.STATUS_OK:
                        scored[fi] = DC.free_score(*raw[b][:5], ids_all[pos:pos + n], *plan, self._table, frame_duration,
                                                   names=[names[int(r)] for r in remap[:len(self._table.names)]])
                    elif want_scores:                         # (the posterior entry refused the path the search gave it)
                        fn = ("wfl_decode_duration_posterior" if free_prior is not None
                              else ("wfl_decode_posterior" if trans is None else "wfl_decode_bigram_posterior"))
                        print(f"{audio_paths[fi]}: no decode scores ({fn} status {raw[b][5] if b in raw else None})")
                pos += n
        return out, scored

    def expected_successions(self, audio_paths, trans, lang_id=None, confidence_threshold=0.0, verbose=True):
        """One Baum-Welch E-step over files without labels, under the grammar and the transition table `trans` ([N, N] float32,
        phonotactics.transition_table) of the bigram search: -> (counts float64 [N, N]: the expected number of runs of symbol q opened
        directly after symbol s, summed over the files in float64 on the host; total_logz; total_lse: the frames' summed log-sum-exp;
        n_frames; skipped: the paths left out).  Symbol 0 is O, symbol 1 + p phoneme p of decode.class_table(labels).  The files are
        forwarded as _decode_viterbi forwards them: a file is one clip, so a run may cross a 30 s seam; the files of a wave go to
        wfl_decode_bigram_counts as one ragged batch (decode.bigram_expected_counts), and one log-sum-exp reduction over the wave's
        logits gives total_lse.  A file whose status is not 0 is skipped with a message."""
        if self._decode_table is None:
            self._decode_table = DC.class_table(self.labels)
        table = self._decode_table
        n = len(table[1]) + 1
        total = np.zeros((n, n), np.float64)
        total_logz = total_lse = 0.0
        n_frames, skipped = 0, []
        for files, by_file in self._file_waves(audio_paths, verbose):
            sel = [fi for fi in files if fi in by_file]
            if not sel:
                continue
            _, rows = self._forward_with_logits(sel, by_file, lang_id, confidence_threshold)
            frames, lg = self._file_rows(rows, by_file, sel)
            d_logz, d_counts, d_st = DC.bigram_expected_counts(lg, frames, table, trans, confidence_threshold)
            f0 = back_to_back(frames)
            d_lse = _clip_lse(lg, f0, f0 + np.asarray(frames, np.int64))
            h = torch.cat([d_logz.double(), d_lse, d_st.double()]).cpu().numpy()
            h_counts = d_counts.cpu().numpy()
            nb = len(sel)
            for b, fi in enumerate(sel):
                if int(h[2 * nb + b]) != DC.STATUS_OK:
                    print(f"{audio_paths[fi]}: no expected successions (wfl_decode_bigram_counts status {int(h[2 * nb + b])}); skipped")
                    skipped.append(audio_paths[fi])
                    continue
                total += h_counts[b].astype(np.float64)
                total_logz += float(h[b])
                total_lse += float(h[nb + b])
                n_frames += int(frames[b])
        return total, total_logz, total_lse, n_frames, skipped

    def expected_durations(self, audio_paths, transcripts, prior, weight=1.0, lang_id=None, confidence_threshold=0.0, verbose=True):
        """One E-step of a duration prior's re-estimation over files with transcripts and no timed labels, under `prior`
        (durations.DurationPrior) at `weight`: -> (counts float64 [len(prior.phonemes), D + 1]: per phoneme the expected number of
        runs of 1 .. D - 1 frames, of D frames or more, and the expected frames past D of those -- the statistics durations.estimate
        counts, for durations.reestimate; total_logz; n_frames; n_tokens; skipped: the paths left out).  transcripts: per file its
        token list, or None.  The files are forwarded and laid out as _label_viterbi lays them out -- a file is one clip across its
        30 s seams, the token alternatives and gap classes are the search's, a token's table row is align.duration_rows' -- and the
        files of a wave go to wfl_align_duration_prior_counts as one ragged batch (align.duration_prior_expected_counts).  Each
        token's row of length posteriors is added, in float64 on the host, to its phoneme's row; a token without a row (-1) goes
        nowhere.  The kernel's logz is on log posteriors already.  A file without a transcript, one whose transcript cannot be
        aligned, or one whose status is not 0 is skipped with one line."""
        from . import durations as DU
        lang_name = self._lang_name(lang_id)
        DU.check(prior, self._names_for(lang_name)[1], frame_duration)
        table = DU.table(prior, weight)
        total = np.zeros((len(prior.phonemes), int(prior.max_frames) + 1), np.float64)
        total_logz, n_frames, n_tokens, skipped = 0.0, 0, 0, []
        for sel, by_file in self._file_waves(audio_paths, verbose):
            sel = [fi for fi in sel if fi in by_file]
            if not sel:
                continue
            free, rows = self._forward_with_logits(sel, by_file, lang_id, confidence_threshold)
            for fi in sel:
                if not transcripts[fi]:
                    print(f"{audio_paths[fi]}: no expected durations (no transcript); skipped")
                    skipped.append(audio_paths[fi])
            with_tr = [fi for fi in sel if transcripts[fi]]
            _, _, plans = self._greedy_and_plans(with_tr, by_file, free, audio_paths, transcripts, lang_name)
            skipped += [audio_paths[fi] for fi in with_tr if fi not in plans]      # (its line: _greedy_and_plans')
            run = [fi for fi in with_tr if fi in plans]
            if not run:
                continue
            frames, lg = self._file_rows(rows, by_file, run)
            durs = [AL.duration_rows(transcripts[fi], prior) for fi in run]
            batch = AL.AlignBatch.of(lg, frames, [plans[fi] for fi in run], [AL.gap_classes(self.labels, transcripts[fi]) for fi in run],
                                     self.labels.index("O"), durs=durs)
            d_logz, d_post, d_st = AL.duration_prior_expected_counts(*batch.args(), batch.durs, table)
            h_logz, h_post, h_st = d_logz.double().cpu().numpy(), d_post.cpu().numpy().astype(np.float64), d_st.cpu().numpy()
            k0 = 0
            for b, fi in enumerate(run):
                n = len(durs[b])
                if int(h_st[b]) != AL.STATUS_OK:
                    print(f"{audio_paths[fi]}: no expected durations (wfl_align_duration_prior_counts status {int(h_st[b])}); skipped")
                    skipped.append(audio_paths[fi])
                else:
                    r = np.asarray(durs[b], np.int64)
                    np.add.at(total, r[r >= 0], h_post[k0:k0 + n][r >= 0])
                    total_logz += float(h_logz[b])
                    n_frames += int(frames[b])
                    n_tokens += n
                k0 += n
        return total, total_logz, n_frames, n_tokens, skipped

    def expected_free_durations(self, audio_paths, trans, prior, weight=1.0, lang_id=None, confidence_threshold=0.0, verbose=True):
        """One E-step over files WITHOUT labels or transcripts, under the explicit-duration grammar of the free decode
        (opts.decode_duration_prior): the transition table `trans` ([N, N] float32, phonotactics.transition_table; None: the flat
        table -postprocess.switch_penalty) and `prior` (durations.DurationPrior) at `weight`.  -> (dur_counts float64
        [len(prior.phonemes), D + 1]: per phoneme the expected number of runs of 1 .. D - 1 frames, of D frames or more, and the
        expected frames past D -- durations.reestimate's statistics; succ float64 [N, N]: expected_successions' table on this
        grammar; total_logz; total_lse; n_frames; skipped).  The files are forwarded and laid out as expected_successions does it: a
        file is one clip across its 30 s seams, the files of a wave one ragged batch (decode.duration_expected_counts,
        wfl_decode_duration_counts).  The tables follow _decode_duration_prior's rule: a symbol's row is the row of its output name, so
        the symbols that share an output name add into one row (float64, on the host); a symbol whose output name the prior lacks
        goes nowhere, one whose row is null is counted under no prior.  A file whose status is not 0 is skipped with one line."""
        from . import durations as DU
        lang_name = self._lang_name(lang_id)
        remap, names = self._names_for(lang_name)
        DU.check(prior, names, frame_duration)
        dur = DU.table(prior, weight)
        if self._decode_table is None:
            self._decode_table = DC.class_table(self.labels)
        table = self._decode_table
        n, D = len(table[1]) + 1, int(prior.max_frames)
        if trans is None:
            trans = np.full((n, n), -float(self.options().switch_penalty), np.float32)
        out = {ph: names[int(remap[i])] for i, ph in enumerate(self._table.names)}
        sym_dur = DC.duration_symbol_rows(prior, table, self.labels, out)
        row_of = {name: i for i, name in enumerate(prior.phonemes)}
        sym_names = [str(self.labels[int(b)])[2:] for b, _ in np.asarray(table[1], np.int32).reshape(-1, 2)]
        acc_row = np.array([row_of.get(out.get(s, s), -1) for s in sym_names], np.int64)
        total = np.zeros((len(prior.phonemes), D + 1), np.float64)
        succ = np.zeros((n, n), np.float64)
        total_logz = total_lse = 0.0
        n_frames, skipped = 0, []
        for files, by_file in self._file_waves(audio_paths, verbose):
            sel = [fi for fi in files if fi in by_file]
            if not sel:
                continue
            _, rows = self._forward_with_logits(sel, by_file, lang_id, confidence_threshold)
            frames, lg = self._file_rows(rows, by_file, sel)
            d_logz, d_succ, d_dur, d_st = DC.duration_expected_counts(lg, frames, table, trans, dur, sym_dur, confidence_threshold)
            f0 = back_to_back(frames)
            d_lse = _clip_lse(lg, f0, f0 + np.asarray(frames, np.int64))
            h = torch.cat([d_logz.double(), d_lse, d_st.double()]).cpu().numpy()
            h_succ, h_dur = d_succ.cpu().numpy(), d_dur.cpu().numpy()
            nb = len(sel)
            for b, fi in enumerate(sel):
                if int(h[2 * nb + b]) != DC.STATUS_OK:
                    print(f"{audio_paths[fi]}: no expected run lengths (wfl_decode_duration_counts status {int(h[2 * nb + b])}); skipped")
                    skipped.append(audio_paths[fi])
                    continue
                np.add.at(total, acc_row[acc_row >= 0], h_dur[b].astype(np.float64)[acc_row >= 0])
                succ += h_succ[b].astype(np.float64)
                total_logz += float(h[b])
                total_lse += float(h[nb + b])
                n_frames += int(frames[b])
        return total, succ, total_logz, total_lse, n_frames, skipped

    def _label_viterbi(self, audio_paths, transcripts, drafts, opts, lang_id, threshold, verbose, prior=None, graphs=None):
        """Files with a transcript, align="viterbi" -> one ViterbiLabel per file.  Their chunks are forwarded with logits (kept on
        the device); the free decode of the same forward gives the greedy result, which the pause rule at the ends needs and which a
        file falls back to (with a message) when its transcript cannot be aligned.  Each file's chunks' valid logits rows are
        concatenated on the device, so one search covers the whole file; the files of a wave are one ragged batch (align.AlignBatch)
        that goes through the stages -- _greedy_and_plans, _clip_constraints, _search, _score, _clip_label -- and only ids / tok /
        score / status and the scoring calls' small tables come back to the host.  drafts: per file its draft segments or None
        (opts.align_draft; the transcript is then the draft's labels).  prior (opts.duration_prior): _duration_prior's pair; the
        search is then the explicit-duration one.  graphs (opts.transcript_variants; None: none): {file: its align.TranscriptGraph}
        for the files whose transcript holds groups -- `transcripts` has their first-variant expansion, for the greedy result and the
        end-pause rule -- which are searched by _search_variants instead; every other file goes through the stages as without."""
        lang_name = self._lang_name(lang_id)
        graphs = graphs or {}
        drafts = drafts if drafts is not None else [None] * len(audio_paths)
        sub_pairs = sub_out = None
        if opts.align_edits or opts.align_insertions:
            sub_names, sub_pairs = AL.substitute_table(self.labels)
            sub_out = AL.substitute_output_names(sub_names, self._table, *self._names_for(lang_name))
        out = []
        for sel, by_file in self._file_waves(audio_paths, verbose):     # a wave's chunks are forwarded and aligned together
            free, rows = self._forward_with_logits(sel, by_file, lang_id, threshold)
            greedy, free_segs, plans = self._greedy_and_plans(sel, by_file, free, audio_paths, transcripts, lang_name,
                                                              opts.filler_token)
            aligned = {}
            run = [fi for fi in sel if fi in plans and fi not in graphs]     # one ragged search over the files that can be aligned
            grun = [fi for fi in sel if fi in plans and fi in graphs]
            if grun:                                         # the files with variants: one ragged search over their graphs
                aligned.update(self._search_variants(grun, graphs, rows, by_file, audio_paths, transcripts, free_segs, lang_name))
            if run:
                paths = [audio_paths[fi] for fi in run]
                frames, lg = self._file_rows(rows, by_file, run)
                chunks = [self._chunk_plan(rows, by_file[fi], fi) for fi in run]
                flags = _clip_flags([transcripts[fi] for fi in run], opts)
                fills = _clip_fillers([transcripts[fi] for fi in run], opts)
                wins, mins = _clip_constraints(paths, frames, chunks, [transcripts[fi] for fi in run],
                                               [drafts[fi] for fi in run], opts, flags)
                batch = AL.AlignBatch.of(lg, frames, [plans[fi] for fi in run], [AL.gap_classes(self.labels, transcripts[fi]) for fi in run],
                                         self.labels.index("O"), wins, mins, flags, fills,
                                         [AL.duration_rows(transcripts[fi], prior[0]) for fi in run] if prior is not None else None)
                found = _search(batch, paths, opts, prior[1] if prior is not None else None)
                scored = _score(found, opts, sub_pairs, prior[1] if prior is not None else None)
                for b, fi in enumerate(run):
                    got = self._clip_label(found, scored, b, chunks[b], transcripts[fi], drafts[fi], free_segs[fi], opts, sub_out,
                                           prior[1] if prior is not None else None)
                    if got is not None:
                        aligned[fi] = got
            for fi in sel:
                out.append(aligned.get(fi, ViterbiLabel(greedy[fi])))
                if fi not in aligned:
                    for key in NOT_ALIGNED_LINES:
                        if R.REPORTS[key].enabled(opts):
                            print(f"{audio_paths[fi]}: {R.REPORTS[key].missing} (the file was not Viterbi-aligned)")
        return out

    def _search_variants(self, grun, graphs, rows, by_file, audio_paths, transcripts, free_segs, lang_name):
        """The files of a wave whose transcripts hold groups -> {file: ViterbiLabel} for those the graph search aligned; one line for
        every other (it keeps its greedy result).  Two calls over the same rows: align.viterbi_align_graph over the graphs, and
        align.viterbi_align over the transcripts as written, whose score the gain is measured against.  Both see the gap classes of
        every slot's name, so SP / AP spelled in any variant count as spelled."""
        remap, names = self._names_for(lang_name)
        slot_alts = {}
        for fi in grun:
            alts, why = AL.token_alternatives(graphs[fi].slots, self._table, remap, names, self.labels)
            if alts is None:
                print(f"{audio_paths[fi]}: viterbi alignment not possible ({why}); using the greedy alignment")
            else:
                slot_alts[fi] = alts
        grun = [fi for fi in grun if fi in slot_alts]
        if not grun:
            return {}
        frames, lg = self._file_rows(rows, by_file, grun)
        gaps = [AL.gap_classes(self.labels, graphs[fi].slots) for fi in grun]
        o_id = self.labels.index("O")
        d_ids, d_tok, d_score, d_st, d_taken = AL.viterbi_align_graph(lg, frames, [slot_alts[fi] for fi in grun],
                                                                      [graphs[fi].preds for fi in grun],
                                                                      [graphs[fi].final for fi in grun], gaps, o_id)
        _, _, w_score, w_st = AL.viterbi_align(lg, frames, [[slot_alts[fi][k] for k in graphs[fi].first] for fi in grun], gaps, o_id)
        ids, tok, taken = d_ids.cpu().numpy(), d_tok.cpu().numpy(), d_taken.cpu().numpy()
        score, status, w_score, w_st = (t.cpu().numpy() for t in (d_score, d_st, w_score, w_st))
        f0 = back_to_back(frames)
        k0 = np.concatenate([[0], np.cumsum([len(graphs[fi].slots) for fi in grun])]).astype(np.int64)
        out = {}
        for b, fi in enumerate(grun):
            g, n, pos = graphs[fi], frames[b], int(f0[b])
            if status[b] != AL.STATUS_OK:
                why = {AL.STATUS_INFEASIBLE: f"no way through the {len(g.groups)} groups' variants fits {n} frames",
                       AL.STATUS_OVER_CAP: f"{len(g.slots)} slots, over the cap of {AL.MAX_SLOTS}"}.get(int(status[b]),
                                                                                                        f"status {int(status[b])}")
                print(f"{audio_paths[fi]}: viterbi alignment not possible ({why}); using the greedy alignment")
                continue
            tk = taken[int(k0[b]):int(k0[b + 1])]
            segs = AL.path_segments(ids[pos:pos + n], tok[pos:pos + n], *self._chunk_plan(rows, by_file[fi], fi), self._table,
                                    slot_alts[fi], g.slots, frame_duration, skipped=1 - tk)
            gain = float(score[b]) - float(w_score[b]) if w_st[b] == AL.STATUS_OK else None
            choices = AL.variant_choices(g, tk, segs, gain)
            print(f"{audio_paths[fi]}: {len(choices)} groups, {sum(r.choice != 0 for r in choices)} not as written, gain "
                  f"{'none' if gain is None else format(gain, '.3f')} nats")
            out[fi] = ViterbiLabel(AL.with_end_pauses(free_segs[fi], segs, transcripts[fi]), None, None, {"variants": choices})
        return out

    def _greedy_and_plans(self, sel, by_file, free, audio_paths, transcripts, lang_name, filler=None):
        """Stage 1, per file of a wave -> (its greedy result: free decode, merge, string match, as _label_files_greedy computes it;
        its merged free segments; the token alternatives of a file whose transcript can be aligned, one line for one that cannot).
        filler (opts.filler_token): the greedy match gets the transcript without its fillers, a filler the placeholder pair."""
        remap, names = self._names_for(lang_name)
        greedy, free_segs, plans = {}, {}, {}
        for fi in sel:
            parts, clock = [], 0.0
            for ci, x in enumerate(by_file[fi]):
                parts.append((*free[(fi, ci)], clock))
                clock += len(x) / self.sr
            segs = free_segs[fi] = self._file_segments(parts, lang_name)
            tr = transcripts[fi]
            spelt = tr if filler is None or not tr else [t for t in tr if t != filler]
            greedy[fi] = AL.with_end_pauses(segs, pp.align_phoneme_list(segs, spelt), spelt)
            alts, why = AL.token_alternatives(tr, self._table, remap, names, self.labels, filler=filler) if tr else (None, None)
            if alts is not None:
                plans[fi] = alts
            elif tr:
                print(f"{audio_paths[fi]}: viterbi alignment not possible ({why}); using the greedy alignment")
        return greedy, free_segs, plans

    def _clip_label(self, found, scored, b, chunk_plan, tr, draft, free_segs, opts, sub_out, dur_table=None):
        """Stage 5: clip b of a searched wave -> its file's ViterbiLabel, or None (with a line) for a clip the search did not align.
        dur_table (opts.duration_prior): the table the clip was searched with."""
        batch = found.batch
        n, pos = batch.frames[b], int(batch.f0[b])
        flags = batch.opts[b] if batch.opts is not None else None
        if found.status[b] != AL.STATUS_OK:
            infeasible = f"{len(tr)} tokens for {n} frames"
            if flags is not None:
                infeasible = f"{len(tr)} tokens need {AL.min_frames_needed(flags)} frames with their optional ones skipped, for {n} frames"
            why = {AL.STATUS_INFEASIBLE: infeasible,
                   AL.STATUS_OVER_CAP: f"{len(tr)} tokens, over the cap of {AL.MAX_TOKENS}"}.get(int(found.status[b]),
                                                                                               f"status {int(found.status[b])}")
            print(f"{found.paths[b]}: viterbi alignment not possible ({why}); using the greedy alignment")
            return None
        tok = found.tok[pos:pos + n]
        left_out, rows = None, {}                         # rows: the clip's side reports, by kind (reports.REPORTS)
        if flags is not None:                             # the clip was searched with skip arcs: which tokens the path left out
            k0 = sum(len(a) for a in batch.alts[:b])
            left_out = found.skipped[k0:k0 + len(tr)]
        fill = batch.fills[b] if batch.fills is not None else None
        segs = AL.path_segments(found.ids[pos:pos + n], tok, *chunk_plan, self._table, batch.alts[b], tr, frame_duration,
                                fillers=fill, skipped=left_out)
        if flags is not None:
            rows["skipped"] = AL.skipped_tokens(left_out, segs, tr)
            print(f"{found.paths[b]}: {len(rows['skipped'])} of {int(sum(flags))} optional tokens skipped")
        moves = draft_moves(draft, segs, tok, batch.wins[b], left_out) if batch.wins[b] is not None else None
        score = None
        if b in scored.raw:
            per_tok = scored.raw[b][2:]
            if left_out is not None:                      # the scores of the kept tokens, one per segment
                per_tok = tuple(a[np.asarray(left_out) == 0] for a in per_tok)
            score = AL.file_score(scored.raw[b][0], scored.raw[b][1], n, *per_tok, segs, frame_duration)
            if b in scored.keep:                          # (scored over the skip lattice: its optional tokens' decisions)
                no_flag = [0] * len(tr)
                rows["optional"] = AL.optional_token_scores(flags if flags is not None else no_flag,
                                                            left_out if left_out is not None else no_flag, scored.keep[b], segs, tr)
        elif (opts.align_scores or opts.duration_scores or opts.optional_scores or opts.filler_scores
              or opts.duration_prior_scores):             # (the scoring entry refused the path the search gave it)
            entry, code = scored.refused.get(b, ("wfl_align_posterior", None))
            print(f"{found.paths[b]}: no alignment scores ({entry} status {code})")
        lab, spans = segs, None
        if fill is not None:                              # a filler's span holds what the file's own free decode found there
            held = {k: AL.filler_segments(g, free_segs) for k, g in enumerate(segs) if fill[k]}
            lab = [x for k, g in enumerate(segs) for x in (held[k] if k in held else [g])]
            spans = rows["fillers"] = [AL.FillerSpan(k, float(segs[k][0]), float(segs[k][1]), int((tok == k).sum()),
                                                     tuple(x[2] for x in held[k])) for k in sorted(held)]
            print(f"{found.paths[b]}: {len(spans)} filler{'s' if len(spans) != 1 else ''} in the transcript")
        if b in scored.edits:
            rows["edits"] = AL.token_edits(scored.edits[b], segs, sub_out)
        if b in scored.insertions:
            rows["insertions"] = AL.place_insertions(scored.insertions[b], segs, sub_out)
        if opts.filler_scores and b in scored.raw:        # one row per filler; a scored file without a filler has none
            rows["filler_scores"] = AL.filler_scores(spans, *scored.raw[b][2:], *scored.ends[b], frame_duration) if spans else []
        if opts.duration_prior_scores and b in scored.ends:
            frames = np.bincount(tok[tok >= 0], minlength=len(batch.durs[b]))
            rows["durations"] = AL.token_durations(score.tokens, frames, batch.durs[b], dur_table, *scored.raw[b][2:], *scored.ends[b],
                                                   frame_duration)
        return ViterbiLabel(AL.with_end_pauses(free_segs, lab, tr), score, moves, rows)


NOT_ALIGNED_LINES = ("optional", "filler_scores", "durations", "edits", "insertions")   # the order a file's lines are printed in


class ViterbiLabel(NamedTuple):
    """Labeler._label_viterbi's record of one file; what does not apply is None."""
    segments: list
    score: AL.FileScore = None      # opts.align_scores / duration_scores, a file that was aligned and scored
    moves: list = None              # [DraftMove], a file aligned inside its draft's windows
    rows: dict = {}                 # the file's side reports, {kind: rows} (reports.REPORTS), of the kinds that apply to the file


class _Searched(NamedTuple):
    """A wave's batch after the search and its fallbacks (_search)."""
    batch: AL.AlignBatch            # its wins / mins: what every clip was last searched with
    paths: list                     # per clip its file's path, for the messages
    ids: np.ndarray                 # viterbi_align's ids / tok / status on the host ...
    tok: np.ndarray
    status: np.ndarray
    d_tok: torch.Tensor             # ... and tok / score on the device, for the scoring calls
    d_score: torch.Tensor
    packed: AL.PackedClips          # what the search ran on; None: packed inside viterbi_align, or a fallback round dropped constraints
    skipped: np.ndarray = None      # viterbi_align_optional's flags of the batch's tokens, clip after clip; None: no clip has optional tokens
    plain: tuple = ()               # the clips a duration prior left no path for: searched again by wfl_align (opts.duration_prior)

    @property
    def ok(self):
        return [b for b in range(len(self.paths)) if self.status[b] == AL.STATUS_OK]


class _Scored(NamedTuple):
    """_score's results, by clip."""
    raw: dict                       # (score, logz, tok_post, start_mean, start_sd) of a clip its scoring entry accepted
    refused: dict                   # (entry, status) of one it refused
    edits: dict                     # the clip's rows of edit_scores' edits
    insertions: dict                # the clip's rows of insertion_scores' ins
    keep: dict                      # optional_posteriors' keep_post of a clip it accepted (opts.optional_scores)
    ends: dict                      # filler_posteriors' (end_mean, end_sd) of a clip it accepted (opts.filler_scores), or
                                    # duration_prior_posteriors' (opts.duration_prior_scores)


def _clip_flags(transcripts, opts):
    """Stage 2 -> per clip the optional flags of its tokens (opts.optional_tokens), None for a clip without any; None: no clip has."""
    if opts.optional_tokens is None:
        return None
    flags = [AL.optional_flags(tr, opts.optional_tokens) for tr in transcripts]
    flags = [f if any(f) else None for f in flags]
    return flags if any(f is not None for f in flags) else None


def _clip_fillers(transcripts, opts):
    """Stage 2 -> per clip the filler flags of its tokens (opts.filler_token), None for a clip without any; None: no clip has."""
    if opts.filler_token is None:
        return None
    flags = [AL.filler_flags(tr, opts.filler_token) for tr in transcripts]
    flags = [f if any(f) else None for f in flags]
    return flags if any(f is not None for f in flags) else None


def _clip_constraints(paths, frames, chunks, transcripts, drafts, opts, flags=None):
    """Stage 2 -> (wins, mins): per clip its draft's start windows and its opts.min_duration in frames, each None where there is
    none or where the host rule align.windows_feasible finds no path (the durations inside the windows), with one line.  flags
    (_clip_flags): a clip with optional tokens keeps its windows whatever that rule says -- it knows no skips; the search's own
    status 1 and _search's safety net decide."""
    wins, mins = [None] * len(paths), [None] * len(paths)
    for b, draft in enumerate(drafts):
        if draft is not None:
            cf, _, cc = chunks[b]
            w = AL.draft_windows(draft, cf, cc, opts.draft_tolerance, frame_duration)
            if (flags is not None and flags[b] is not None) or AL.windows_feasible(frames[b], w):
                wins[b] = w
            else:
                print(f"{paths[b]}: {DRAFT_INFEASIBLE}")
    if opts.min_duration is not None:
        for b, tr in enumerate(transcripts):
            d = AL.min_frames_for(tr, opts.min_duration, frame_duration)
            w = wins[b] if wins[b] is not None else [AL.OPEN_WINDOW] * len(d)
            if AL.windows_feasible(frames[b], w, d):
                mins[b] = d
            elif frames[b] >= len(d):                     # (fewer frames than tokens: the search's own status 1, as without)
                print(f"{paths[b]}: {MIN_DURATION_INFEASIBLE}")
    return wins, mins


def _search(batch, paths, opts, dur_table=None) -> _Searched:
    """Stage 3: the search over the whole batch, packed here when scores or edits are to run on the same tables (the durations only
    with opts.duration_scores; without, they go to viterbi_align beside a PackedClips that has none), then the safety net: a clip
    the kernel found no path for inside its constraints is searched again, first without its durations, then without its windows.
    dur_table (opts.duration_prior): the prior's table; the batch's clips (their rows in batch.durs) go through the explicit-duration
    search, and a clip it has no path for is aligned again by the plain search, with one line."""
    if batch.durs is not None:                            # (the options refuse drafts, durations, optional tokens, fillers and scores
        d_ids, d_tok, d_score, d_st = AL.viterbi_align_duration_prior(*batch.args(), batch.durs, dur_table)       # beside a prior)
        status = d_st.cpu().numpy()
        again = [b for b in range(len(paths)) if status[b] != AL.STATUS_OK]
        if again:
            for b in again:
                print(f"{paths[b]}: {DURATION_PRIOR_INFEASIBLE}")
            sub = batch.select(again)
            r_ids, r_tok, r_score, r_st = AL.viterbi_align(*sub.args(), frame_offsets=sub.f0)
            for j, b in enumerate(again):
                rows_b = slice(int(batch.f0[b]), int(batch.f0[b]) + batch.frames[b])
                d_ids[rows_b], d_tok[rows_b] = r_ids[rows_b], r_tok[rows_b]
                d_score[b], d_st[b] = r_score[j], r_st[j]
            status = d_st.cpu().numpy()
        return _Searched(batch, paths, d_ids.cpu().numpy(), d_tok.cpu().numpy(), status, d_tok, d_score, None, plain=tuple(again))
    scoring = opts.align_scores or opts.align_edits or opts.align_insertions
    packed = batch.pack(opts.duration_scores) if scoring or (opts.duration_scores and batch.min_frames is not None) else None
    d_skip = None
    if batch.fillers is not None:                         # (the options refuse drafts, durations, optional tokens and scores beside a
        d_ids, d_tok, d_score, d_st = AL.viterbi_align_filler(*batch.args(), batch.fillers, opts.filler_penalty)     # filler: one call)
    elif batch.optional is not None:                      # (the options refuse durations and scores beside optional tokens)
        d_ids, d_tok, d_score, d_st, d_skip = AL.viterbi_align_optional(*batch.args(), batch.optional, opts.skip_penalty,
                                                                        windows=batch.windows)
        k0 = np.concatenate([[0], np.cumsum([len(a) for a in batch.alts])]).astype(np.int64)
    else:
        d_ids, d_tok, d_score, d_st = AL.viterbi_align(*batch.args(), packed=packed, windows=batch.windows, min_frames=batch.min_frames)
    status = d_st.cpu().numpy()
    for _ in range(2):
        again = [b for b in range(len(paths))
                 if (batch.wins[b] is not None or batch.mins[b] is not None) and status[b] == AL.STATUS_INFEASIBLE]
        if not again:
            break
        for b in again:
            if batch.mins[b] is not None:
                print(f"{paths[b]}: {MIN_DURATION_INFEASIBLE}")
                batch.mins[b] = None
            else:
                print(f"{paths[b]}: {DRAFT_INFEASIBLE}")
                batch.wins[b] = None
        sub = batch.select(again)                         # (its clips keep their optional flags when they drop their windows)
        if sub.optional is not None:
            r_ids, r_tok, r_score, r_st, r_skip = AL.viterbi_align_optional(*sub.args(), sub.optional, opts.skip_penalty,
                                                                            frame_offsets=sub.f0, windows=sub.windows)
            j0 = 0
            for b in again:
                d_skip[int(k0[b]):int(k0[b + 1])] = r_skip[j0:j0 + int(k0[b + 1] - k0[b])]
                j0 += int(k0[b + 1] - k0[b])
        else:
            r_ids, r_tok, r_score, r_st = AL.viterbi_align(*sub.args(), frame_offsets=sub.f0, windows=sub.windows)
        for j, b in enumerate(again):
            rows_b = slice(int(batch.f0[b]), int(batch.f0[b]) + batch.frames[b])
            d_ids[rows_b], d_tok[rows_b] = r_ids[rows_b], r_tok[rows_b]
            d_score[b], d_st[b] = r_score[j], r_st[j]
        status = d_st.cpu().numpy()
        packed = None                                     # (packed for the constraints that were dropped)
    return _Searched(batch, paths, d_ids.cpu().numpy(), d_tok.cpu().numpy(), status, d_tok, d_score, packed,
                     d_skip.cpu().numpy() if d_skip is not None else None)


def _score(found, opts, sub_pairs, dur_table=None) -> _Scored:
    """Stage 4: edits, insertions, posteriors, duration posteriors of the clips the search aligned, each call on a sub-batch and on
    the lattice its clips were searched on (AlignBatch.scored_on: the search's PackedClips or tables packed again).  dur_table
    (opts.duration_prior): the table of the explicit-duration search, for opts.duration_prior_scores."""
    scored = _Scored({}, {}, {}, {}, {}, {})
    ok = found.ok
    if not ok:
        return scored
    if opts.align_scores or opts.align_edits or opts.align_insertions:
        sub, packed = found.batch.scored_on(ok, found.packed, False)
    if opts.align_edits:
        scored.edits.update(_edit_rows(found, sub, packed, AL.edit_scores, AL.edits_workspace_bytes, 0, "edits", "wfl_align_edits",
                                       sub_pairs))
    if opts.align_insertions:                             # (a clip's N + 1 places: one row more than its tokens)
        scored.insertions.update(_edit_rows(found, sub, packed, AL.insertion_scores, AL.insertions_workspace_bytes, 1, "insertions",
                                            "wfl_align_insertions", sub_pairs))
    if opts.align_scores:
        d_post = AL.alignment_posteriors(*sub.args(), found.d_tok, frame_offsets=sub.f0, packed=packed)
        _take_posteriors(found, ok, d_post, "wfl_align_posterior", scored)
    if opts.duration_scores:
        # every clip on the lattice it was searched on: with its durations, or -- where they were dropped -- without
        for with_min in (True, False):
            part = [b for b in ok if (found.batch.mins[b] is not None) == with_min]
            if not part:
                continue
            sub, packed = found.batch.scored_on(part, found.packed, with_min)
            if not with_min:
                for b in part:
                    print(f"{found.paths[b]}: {DURATION_SCORES_PLAIN}")
            d_post = (AL.duration_posteriors if with_min else AL.alignment_posteriors)(*sub.args(), found.d_tok, frame_offsets=sub.f0,
                                                                                     packed=packed)
            _take_posteriors(found, part, d_post, "wfl_align_min_duration_posterior" if with_min else "wfl_align_posterior", scored)
    if opts.optional_scores:
        # the clips searched with flags, over the skip lattice and on the windows they ended the search with (after _search's
        # fallback has dropped any); a batch none of whose clips has a flag was searched by wfl_align, and is scored on that lattice
        sub = found.batch.select(ok)
        packed = sub.pack(False)
        if found.batch.optional is not None:
            d = AL.optional_posteriors(*sub.args(), sub.opts, found.d_tok, opts.skip_penalty, frame_offsets=sub.f0, packed=packed)
            _take_posteriors(found, ok, (d[0], d[2], d[3], d[4], d[5]), "wfl_align_optional_posterior", scored)
            h_keep, k0 = d[1].cpu().numpy(), 0
            for b in ok:
                if b in scored.raw:
                    scored.keep[b] = h_keep[k0:k0 + len(found.batch.alts[b])]
                k0 += len(found.batch.alts[b])
        else:
            d_post = AL.alignment_posteriors(*sub.args(), found.d_tok, frame_offsets=sub.f0, packed=packed)
            _take_posteriors(found, ok, d_post, "wfl_align_posterior", scored)
            for b in ok:
                if b in scored.raw:
                    scored.keep[b] = np.ones(len(found.batch.alts[b]), np.float32)
    if opts.filler_scores:
        # every clip on the lattice it was searched on: a clip with a filler over the filler lattice, with the flags and the penalty of
        # its search; a clip without one was searched on wfl_align's lattice (wfl_align_filler's with no flag set) and is scored there
        fills = found.batch.fills or [None] * len(found.paths)
        for with_fill in (True, False):
            part = [b for b in ok if (fills[b] is not None and any(fills[b])) == with_fill]
            if not part:
                continue
            sub = found.batch.select(part)
            packed = sub.pack(False)
            if with_fill:
                d = AL.filler_posteriors(*sub.args(), sub.fills, found.d_tok, opts.filler_penalty, frame_offsets=sub.f0, packed=packed)
                _take_posteriors(found, part, (d[0], d[1], d[2], d[3], d[6]), "wfl_align_filler_posterior", scored)
                h_end, k0 = torch.stack([d[4], d[5]]).cpu().numpy(), 0
                for b in part:
                    n = len(found.batch.alts[b])
                    if b in scored.raw:
                        scored.ends[b] = (h_end[0, k0:k0 + n], h_end[1, k0:k0 + n])
                    k0 += n
            else:
                for b in part:
                    print(f"{found.paths[b]}: {FILLER_SCORES_PLAIN}")
                d_post = AL.alignment_posteriors(*sub.args(), found.d_tok, frame_offsets=sub.f0, packed=packed)
                _take_posteriors(found, part, d_post, "wfl_align_posterior", scored)
    if opts.duration_prior_scores and found.batch.durs is not None:
        # every clip on the lattice it was searched on: under the prior over the explicit-duration lattice, with the rows and the table
        # of its search; a clip the prior left no path for was searched by wfl_align and is scored there
        for with_prior in (True, False):
            part = [b for b in ok if (b not in found.plain) == with_prior]
            if not part:
                continue
            sub = found.batch.select(part)
            packed = sub.pack(False)
            if with_prior:
                d = AL.duration_prior_posteriors(*sub.args(), sub.durs, dur_table, found.d_tok, frame_offsets=sub.f0, packed=packed)
                _take_posteriors(found, part, (d[0], d[1], d[2], d[3], d[6]), "wfl_align_duration_prior_posterior", scored)
                h_end, k0 = torch.stack([d[4], d[5]]).cpu().numpy(), 0
                for b in part:
                    n = len(found.batch.alts[b])
                    if b in scored.raw:
                        scored.ends[b] = (h_end[0, k0:k0 + n], h_end[1, k0:k0 + n])
                    k0 += n
            else:
                for b in part:
                    print(f"{found.paths[b]}: {DURATION_PRIOR_SCORES_PLAIN}")
                d_post = AL.alignment_posteriors(*sub.args(), found.d_tok, frame_offsets=sub.f0, packed=packed)
                _take_posteriors(found, part, d_post, "wfl_align_posterior", scored)
    return scored


def _edit_rows(found, sub, packed, scorer, workspace_bytes, extra, what, entry, sub_pairs):
    """-> {clip: its n_tok + extra rows of scorer's table} for the aligned clips `sub`, in groups under EDITS_WORKSPACE_LIMIT."""
    n_tok = [len(a) for a in sub.alts]
    ok, out = found.ok, {}
    for grp in AL.edit_groups(sub.frames, n_tok, workspace_bytes=workspace_bytes):
        gsub, gpack = sub.scored_on(grp, packed, False)
        _, d_ed, d_est = scorer(*gsub.args(), sub_pairs, packed=gpack)
        h_ed, h_est = d_ed.cpu().numpy(), d_est.cpu().numpy()
        k0 = 0
        for q, j in enumerate(grp):
            if h_est[q] == AL.STATUS_OK:
                out[ok[j]] = h_ed[k0:k0 + n_tok[j] + extra]
            else:
                print(f"{found.paths[ok[j]]}: no transcript {what} ({entry} status {int(h_est[q])})")
            k0 += n_tok[j] + extra
    return out


def _take_posteriors(found, clips, d_post, entry, scored):
    """A scoring call's tensors for `clips` -> scored.raw / scored.refused, in one copy to the host."""
    n_tok = [len(found.batch.alts[b]) for b in clips]
    nt, n = sum(n_tok), len(clips)
    h = torch.cat([found.d_score[clips], *d_post[:4], d_post[4].to(torch.float32)]).cpu().numpy()      # one copy
    h_score, h_logz, h_st = h[:n], h[n:2 * n], h[2 * n + 3 * nt:]
    k0 = 0
    for j, b in enumerate(clips):
        if h_st[j] != AL.STATUS_OK:
            scored.refused[b] = (entry, int(h_st[j]))
        else:
            scored.raw[b] = (h_score[j], h_logz[j]) + tuple(h[2 * n + q * nt + k0:2 * n + q * nt + k0 + n_tok[j]] for q in range(3))
        k0 += n_tok[j]


def _clip_lse(lg, starts, ends):
    """Per clip the sum of the log-sum-exp of its frames' logits, frames [start, end) of `lg` (int64 host arrays) -> float64 on the
    device: path_log_posterior's third term, which the ABI has no output for.  One fp32 reduction over the wave's logits, then
    differences of one running sum in double."""
    run = torch.cat([lg.new_zeros(1, dtype=torch.float64), torch.logsumexp(lg, dim=1).double().cumsum(0)])
    return run[torch.from_numpy(ends).to(lg.device)] - run[torch.from_numpy(starts).to(lg.device)]


MIN_DURATION_INFEASIBLE = ("no path gives every token its minimum duration (postprocess.min_duration: too many tokens for the frames, or "
                           "for the draft's windows); aligning the transcript without minimum durations")
DURATION_PRIOR_INFEASIBLE = ("no path of finite score under the duration prior (postprocess.duration_prior: the table forbids every "
                             "segmentation of these frames, or the search refused the clip); aligning the transcript without the prior")
DURATION_SCORES_PLAIN = ("scored without minimum durations (postprocess.duration_scores: the file was searched without them, and a "
                         "score speaks of the lattice its search ran on)")
DURATION_PRIOR_SCORES_PLAIN = ("scored by wfl_align_posterior (postprocess.duration_prior_scores: the prior left the file no path, so it "
                               "was searched without the prior, and a score speaks of the lattice its search ran on)")
FILLER_SCORES_PLAIN = ("scored by wfl_align_posterior (postprocess.filler_scores: the transcript has no filler, so the file was searched "
                       "on the lattice without a filler emission, and a score speaks of the lattice its search ran on)")
DRAFT_INFEASIBLE = ("no path opens every token inside its draft window (two starts on one frame, or more tokens than frames in between); "
                    "aligning the draft's transcript without windows")


class DraftMove(NamedTuple):
    index: int              # the token's place in the transcript
    token: str
    draft_start_s: float
    start_s: float          # the token's start in the new .lab
    on_edge: bool           # the token opens on the first or the last frame of its window: it wants to be elsewhere

    @property
    def move_s(self) -> float:
        return self.start_s - self.draft_start_s


def draft_moves(draft, segments, tok, windows, skipped=None):
    """Per token of a file aligned inside its draft's windows -> [DraftMove]: draft (start_s, end_s, label) and segments
    (path_segments) one per token in order, tok the file's per-frame token index, windows the (lo, hi) rows the search was held to.
    skipped (align.viterbi_align_optional's flags of the tokens; None: none): the segments are the kept tokens', and so are the rows."""
    tok = np.asarray(tok)
    opens = np.nonzero((tok >= 0) & (np.concatenate([[-1], tok[:-1]]) != tok))[0]        # one frame per token, in order
    first = {int(tok[t]): int(t) for t in opens[::-1]}
    kept = [k for k in range(len(draft)) if skipped is None or not int(skipped[k])]
    return [DraftMove(k, str(seg[2]), float(draft[k][0]), float(seg[0]), first[k] in (int(windows[k][0]), int(windows[k][1])))
            for k, seg in zip(kept, segments)]


def format_draft_moves_tsv(named_moves) -> str:
    """`draft_moves.tsv` of a folder: [(file name, [DraftMove])] -> one line per token, `file index token draft_start start move_s
    on_edge`, draft_start / start being the integers a .lab line carries.  on_edge = 1 is the QA list: a token pressed against its
    window wants to leave the neighbourhood its draft put it in."""
    lines = ["# file\tindex\ttoken\tdraft_start\tstart\tmove_s\ton_edge"]
    for name, ms in named_moves:
        for m in ms:
            lines.append(f"{name}\t{m.index}\t{m.token}\t{_lab_int(m.draft_start_s)}\t{_lab_int(m.start_s)}\t{m.move_s:+.4f}\t"
                         f"{int(m.on_edge)}")
    return "\n".join(lines) + "\n"


def _read_draft(audio_path, draft_dir, forced):
    """The draft of X.wav: DIR/X.lab -> its segments, or None when there is none (no file, or a file without a segment).  forced: the
    file's `{audio}.txt` transcript or None; one line when it spells something else than the draft, which wins."""
    lab = os.path.join(draft_dir, os.path.splitext(os.path.basename(audio_path))[0] + ".lab")
    if not os.path.isfile(lab):
        return None
    draft = AL.read_draft(lab)
    if not draft:
        print(f"{audio_path}: the draft {lab} holds no segment; the file is handled without it")
        return None
    if forced is not None and forced != [s[2] for s in draft]:
        print(f"{audio_path}: the transcript beside the audio spells something else than the draft {lab}; the draft wins")
    return draft


def _read_variants(audio_paths, forced, output_names):
    """opts.transcript_variants: the files whose transcript holds a group -> {file: its align.TranscriptGraph}; forced[fi] of such a
    file becomes its first-variant expansion, the transcript as written.  A malformed transcript is a ValueError that names the
    file and the place; so is an output name of the label set that holds a syntax character."""
    clash = AL.variant_name_collisions(output_names)
    if clash:
        raise ValueError(f"transcript_variants: {', '.join(repr(n) for n in clash)} of this model's label set holds one of "
                         f"{' '.join(AL.VARIANT_CHARS)}, which are syntax with the option on")
    graphs = {}
    for fi, tr in enumerate(forced):
        if tr and AL.has_variants(tr):
            txt = audio_paths[fi].replace(".wav", ".txt")
            notes = []
            try:
                g = AL.compile_graph(AL.parse_variants(tr, notes))
            except ValueError as err:
                raise ValueError(f"{txt}: {err}") from None
            for line in notes:
                print(f"{txt}: {line}")
            graphs[fi] = g
            forced[fi] = [g.slots[k] for k in g.first]
    return graphs


def _read_forced(audio_path, verbose):
    """`{audio}.txt` forced phoneme list (infer.py:193, 210-215)."""
    txt = audio_path.replace(".wav", ".txt")
    if txt == audio_path or not os.path.exists(txt):
        return None
    forced = []
    with open(txt, "r", encoding="utf-8") as f:
        for line in f:
            forced.extend(line.strip().split())
    if verbose:
        print(f"Loaded forced phoneme list with {len(forced)} phonemes.")
    return forced


_LABELERS = {}


def _labeler(config_path, checkpoint_path, device):
    key = (os.path.abspath(str(config_path)), os.path.abspath(str(checkpoint_path)), str(device))
    if key not in _LABELERS:
        _LABELERS[key] = Labeler(config_path, checkpoint_path, device)
    return _LABELERS[key]


def _write_lab(path, segments):
    """save_lab (utils.py:76-81) with the text produced by the native formatter (wfl_host_format_lab: truncating int(t * 1e7))."""
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    with open(path, "wb") as f:
        f.write(npost.format_lab_tuples(segments))
    print(f"Predictions saved to: {path}")


def _refuse_before_load(config_path, **given):
    """The refusal before any model is loaded: the request resolved against the `postprocess` section of the config file, when that
    file exists ({} otherwise; such a call fails at the model load).  The options that labelling uses are the Labeler's own
    (Labeler.options: a cached Labeler keeps the config it was loaded with)."""
    cfg = load_config(config_path) if os.path.isfile(str(config_path)) else None
    resolve((cfg or {}).get("postprocess"), **given)


def _lab_int(t):
    """The integer a .lab line carries for a time (the native formatter's truncating int(t * 1e7))."""
    return int(npost.format_lab_tuples([(t, t, "x")]).split()[0])


def format_scores_tsv(score) -> str:
    """`{stem}.scores.tsv` of one Viterbi-aligned file (align.FileScore): a `#` header line with the file's figures, then one line
    per transcript token, `start end token posterior start_sd_s start_shift_s`, start / end being the integers of the token's .lab
    line."""
    lines = [f"# path_log_posterior={score.path_log_posterior:.4f}\tmean_frame_logprob={score.mean_frame_logprob:.6f}\t"
             f"mean_frame_logz={score.mean_frame_logz:.6f}\tmin_posterior={score.min_posterior:.6f}"]
    for t in score.tokens:
        lines.append(f"{_lab_int(t.start_s)}\t{_lab_int(t.end_s)}\t{t.token}\t{t.posterior:.6f}\t{t.start_sd_s:.4f}\t"
                     f"{t.start_shift_s:+.4f}")
    return "\n".join(lines) + "\n"


def format_review_tsv(named_scores) -> str:
    """`alignment_scores.tsv` of a folder: [(file name, FileScore)] -> one line per aligned file, the weakest first (ascending
    min_posterior; ties by name): the review list."""
    rows = sorted(named_scores, key=lambda r: (r[1].min_posterior, r[0]))
    lines = ["# file\tmin_posterior\tpath_log_posterior\tmean_frame_logprob\tmean_frame_logz\ttokens"]
    for name, sc in rows:
        lines.append(f"{name}\t{sc.min_posterior:.6f}\t{sc.path_log_posterior:.4f}\t{sc.mean_frame_logprob:.6f}\t"
                     f"{sc.mean_frame_logz:.6f}\t{len(sc.tokens)}")
    return "\n".join(lines) + "\n"


DECODE_SCORES_NOTE = "runs are the path's runs before merge_segments and any transcript match"


def format_decode_scores_tsv(score, lab_lines) -> str:
    """`{stem}.decode_scores.tsv` of one file the grammar search decoded (decode.FreeScore): a `#` header line with the file's four
    figures, the number of runs beside the number of lines of the .lab, and the note that the two may differ; then one line per run of
    the path, `start end phoneme posterior start_posterior min_frame_posterior`, start / end being the integers a .lab line carries
    for the run's times."""
    lines = [f"# path_log_posterior={score.path_log_posterior:.4f}\tmean_frame_logprob={score.mean_frame_logprob:.6f}\t"
             f"legal_log_mass_per_frame={score.legal_log_mass_per_frame:.6f}\tmin_posterior={score.min_posterior:.6f}\t"
             f"runs={len(score.runs)} lab_lines={int(lab_lines)}\t{DECODE_SCORES_NOTE}"]
    for r in score.runs:
        lines.append(f"{_lab_int(r.start_s)}\t{_lab_int(r.end_s)}\t{r.phoneme}\t{r.posterior:.6f}\t{r.start_posterior:.6f}\t"
                     f"{r.min_frame_posterior:.6f}")
    return "\n".join(lines) + "\n"


def format_decode_review_tsv(named_scores) -> str:
    """`decode_scores.tsv` of a folder: [(file name, FreeScore)] -> one line per scored file, the weakest first (ascending
    min_posterior; ties by name): the review list."""
    rows = sorted(named_scores, key=lambda r: (r[1].min_posterior, r[0]))
    lines = ["# file\tmin_posterior\tpath_log_posterior\tmean_frame_logprob\tlegal_log_mass_per_frame\truns"]
    for name, sc in rows:
        lines.append(f"{name}\t{sc.min_posterior:.6f}\t{sc.path_log_posterior:.4f}\t{sc.mean_frame_logprob:.6f}\t"
                     f"{sc.legal_log_mass_per_frame:.6f}\t{len(sc.runs)}")
    return "\n".join(lines) + "\n"


def _write_text(path, text, what):
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    with open(path, "w", encoding="utf-8") as f:
        f.write(text)
    print(f"{what} saved to: {path}")


def scores_path(lab_path):
    return os.path.splitext(lab_path)[0] + ".scores.tsv"


def decode_scores_path(lab_path):
    return os.path.splitext(lab_path)[0] + ".decode_scores.tsv"


def _write_reports(lab_path, reports, fi):
    """File fi's side reports beside its .lab, one file per enabled kind the file has rows of, in reports.REPORTS' order."""
    for key, by_file in reports.rows.items():
        if by_file.get(fi) is not None:
            _write_text(R.file_path(key, lab_path), R.file_text(key, by_file[fi]), R.KINDS[key].what)


def _write_score(lab_path, segments, score):
    """The scores file of one labelled file beside its .lab, by the kind of its score (None: no file)."""
    if isinstance(score, DC.FreeScore):
        _write_text(decode_scores_path(lab_path), format_decode_scores_tsv(score, len(segments)), "Decode scores")
    elif score is not None:
        _write_text(scores_path(lab_path), format_scores_tsv(score), "Alignment scores")


def infer_audio(audio_path, config_path="config.yaml", checkpoint_path="best_model.pt", output_lab_path=None, device="cuda",
                lang_id=None, sample=False, top_k=0, top_p=0.0, temperature=1.0, confidence_threshold=0.0, align=None,
                align_scores=None, decode=None, switch_penalty=None, decode_scores=None, phoneme_bigram=None, bigram_weight=None,
                align_draft=None, draft_tolerance=None, align_edits=None, align_insertions=None, min_duration=None,
                duration_scores=None, optional_tokens=None, skip_penalty=None, optional_scores=None, filler_token=None,
                filler_penalty=None, filler_scores=None, duration_prior=None, duration_prior_weight=None,
                duration_prior_scores=None, decode_duration_prior=None, decode_duration_prior_weight=None,
                decode_duration_scores=None, transcript_variants=None, bigram_scores=None):
    """align: "greedy" | "viterbi" | None (config postprocess.align, else greedy): how a `{audio}.txt` transcript is aligned
    (Labeler.label_files).  align_scores (viterbi only; None: config postprocess.align_scores): also write `{stem}.scores.tsv`
    beside the .lab when the file was Viterbi-aligned (format_scores_tsv).  decode: "argmax" | "viterbi" | None (config
    postprocess.decode, else argmax) and switch_penalty (nats, >= 0; None: config postprocess.switch_penalty, else 0): how the free
    decode is made (Labeler.label_files).  decode_scores (decode viterbi only; None: config postprocess.decode_scores): also write
    `{stem}.decode_scores.tsv` beside the .lab when the grammar search decoded the file (format_decode_scores_tsv).  phoneme_bigram /
    bigram_weight (decode viterbi only; None: config postprocess.phoneme_bigram / postprocess.bigram_weight): the phone-bigram prior
    of the search (Labeler.label_files).  bigram_scores (with a phoneme_bigram only; None: config postprocess.bigram_scores):
    decode_scores for a bigram decode, the same `{stem}.decode_scores.tsv`.  align_draft / draft_tolerance (align viterbi only; None:
    config postprocess.align_draft / postprocess.draft_tolerance): refine the draft DIR/{stem}.lab inside per-token start windows
    (Labeler.label_files).  align_edits (align viterbi only; None: config postprocess.align_edits): also write `{stem}.edits.tsv`
    beside the .lab when the file was Viterbi-aligned: per token the best and second-best substitute, the deletion, their log
    likelihood ratios and a flag (reports.REPORTS["edits"]).  align_insertions (align viterbi only; None: config
    postprocess.align_insertions): also write `{stem}.insertions.tsv` beside the .lab when the file was Viterbi-aligned: per place of
    the transcript the best and second-best phoneme to insert, their log likelihood ratios and a flag (reports.REPORTS["insertions"]).
    min_duration (align viterbi only; None: config postprocess.min_duration): seconds, or {token name: seconds, "default": seconds}:
    the least time a transcript token occupies in the search (Labeler.label_files).  duration_scores (with a min_duration only; None:
    config postprocess.duration_scores): align_scores for that search, the same `{stem}.scores.tsv`, summed over the
    minimum-duration lattice (align.duration_posteriors).  optional_tokens / skip_penalty (align viterbi only; None: config
    postprocess.optional_tokens / postprocess.skip_penalty): the transcript tokens a path may leave out, [NAME, ...] or "*", and the
    nats each skipped one costs (Labeler.label_files); the .lab lacks the skipped tokens and `{stem}.skipped.tsv` lists them
    (reports.REPORTS["skipped"]).  optional_scores (with optional_tokens only; None: config postprocess.optional_scores): also write
    `{stem}.scores.tsv` for the kept tokens, summed over the skip lattice, and `{stem}.optional.tsv`, one row per optional token of
    the transcript with the posterior probability that it is present (align.optional_posteriors, reports.REPORTS["optional"]).
    filler_token / filler_penalty (align viterbi only; None: config postprocess.filler_token / postprocess.filler_penalty): the
    transcript token that matches anything and the nats it pays per frame (Labeler.label_files); in the .lab its span holds what
    the free decode found there, and `{stem}.fillers.tsv` lists the spans (reports.REPORTS["fillers"]).  filler_scores (with a
    filler_token only; None: config postprocess.filler_scores): also write `{stem}.scores.tsv`, one row per transcript token summed
    over the lattice the file was searched on, and `{stem}.filler_scores.tsv`, one row per filler with the posterior of its span and
    the mean shift and spread of both its ends (align.filler_posteriors, reports.REPORTS["filler_scores"]); the .lab and
    `{stem}.fillers.tsv` are what they are without it.  duration_prior / duration_prior_weight (align viterbi only; None: config
    postprocess.duration_prior / postprocess.duration_prior_weight): the phoneme duration prior of the explicit-duration search and
    what its log probabilities are multiplied by (Labeler.label_files).  duration_prior_scores (with a duration_prior only; None:
    config postprocess.duration_prior_scores): also write `{stem}.scores.tsv`, one row per transcript token summed over the lattice
    the file was searched on, and, for a file searched under the prior, `{stem}.durations.tsv`, one row per token with its length,
    the prior's log probability of it, the posterior of its run, the shift and spread of both its ends and its expected length
    (align.duration_prior_posteriors, reports.REPORTS["durations"]); the .lab is what it is without it.  decode_duration_prior /
    decode_duration_prior_weight (decode viterbi only; None: config postprocess.decode_duration_prior /
    postprocess.decode_duration_prior_weight): the phoneme duration prior of the FREE decode's explicit-duration search and what its log
    probabilities are multiplied by (Labeler.label_files).  decode_duration_scores (with a decode_duration_prior only; None: config
    postprocess.decode_duration_scores): decode_scores for the duration-prior decode -- the same `{stem}.decode_scores.tsv`, from
    decode.decode_posteriors_duration over the explicit-duration grammar of that search."""
    given = dict(align=align, align_scores=align_scores, decode=decode, switch_penalty=switch_penalty, decode_scores=decode_scores,
                 phoneme_bigram=phoneme_bigram, bigram_weight=bigram_weight, bigram_scores=bigram_scores, align_draft=align_draft,
                 draft_tolerance=draft_tolerance, align_edits=align_edits, align_insertions=align_insertions, min_duration=min_duration,
                 duration_scores=duration_scores, optional_tokens=optional_tokens, skip_penalty=skip_penalty,
                 optional_scores=optional_scores, filler_token=filler_token, filler_penalty=filler_penalty,
                 filler_scores=filler_scores, duration_prior=duration_prior, duration_prior_weight=duration_prior_weight,
                 duration_prior_scores=duration_prior_scores, decode_duration_prior=decode_duration_prior,
                 decode_duration_prior_weight=decode_duration_prior_weight, decode_duration_scores=decode_duration_scores,
                 transcript_variants=transcript_variants)
    _refuse_before_load(config_path, **given)
    lab = _labeler(config_path, checkpoint_path, device)
    opts = lab.options(**given)
    reports = R.Reports.for_options(opts)
    (segments,), (score,) = lab._label_scored([audio_path], opts, lang_id, confidence_threshold, True, reports)
    if output_lab_path:
        if os.path.abspath(output_lab_path) == os.path.abspath(audio_path):
            # the reference would truncate the input WAV here (infer.py:410-411 + utils.py:77)
            output_lab_path = os.path.splitext(audio_path)[0] + ".lab"
        _write_lab(output_lab_path, segments)
        _write_score(output_lab_path, segments, score)
        _write_reports(output_lab_path, reports, 0)
    return segments


def infer_folder(folder_path: str, config_path: str = "config.yaml", checkpoint_path: str = "best_model.pt",
                 output_dir: str = "outputs", device: str = "cuda", lang_id: int = None, sample=False, top_k=0, top_p=0.0,
                 temperature=1.0, confidence_threshold=0.0, align=None, align_scores=None, decode=None, switch_penalty=None,
                 decode_scores=None, phoneme_bigram=None, bigram_weight=None, align_draft=None, draft_tolerance=None,
                 align_edits=None, align_insertions=None, min_duration=None, duration_scores=None, optional_tokens=None,
                 skip_penalty=None, optional_scores=None, filler_token=None, filler_penalty=None, filler_scores=None,
                 duration_prior=None, duration_prior_weight=None, duration_prior_scores=None,
                 decode_duration_prior=None, decode_duration_prior_weight=None, decode_duration_scores=None,
                 transcript_variants=None, bigram_scores=None):
    given = dict(align=align, align_scores=align_scores, decode=decode, switch_penalty=switch_penalty, decode_scores=decode_scores,
                 phoneme_bigram=phoneme_bigram, bigram_weight=bigram_weight, bigram_scores=bigram_scores, align_draft=align_draft,
                 draft_tolerance=draft_tolerance, align_edits=align_edits, align_insertions=align_insertions, min_duration=min_duration,
                 duration_scores=duration_scores, optional_tokens=optional_tokens, skip_penalty=skip_penalty,
                 optional_scores=optional_scores, filler_token=filler_token, filler_penalty=filler_penalty,
                 filler_scores=filler_scores, duration_prior=duration_prior, duration_prior_weight=duration_prior_weight,
                 duration_prior_scores=duration_prior_scores, decode_duration_prior=decode_duration_prior,
                 decode_duration_prior_weight=decode_duration_prior_weight, decode_duration_scores=decode_duration_scores,
                 transcript_variants=transcript_variants)
    _refuse_before_load(config_path, **given)
    wav_files = sorted(f for f in os.listdir(folder_path) if f.lower().endswith(".wav"))
    os.makedirs(output_dir, exist_ok=True)
    # one process per GPU: every rank labels its own share of the files and writes its own .lab files (no collective)
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1:
        from .dist import shard_items
        sizes = [os.path.getsize(os.path.join(folder_path, f)) for f in wav_files]
        wav_files = [wav_files[i] for i in shard_items(sizes, world)[rank]]
    lab = _labeler(config_path, checkpoint_path, device)
    paths = [os.path.join(folder_path, f) for f in wav_files]
    opts = lab.options(**given)
    reports = R.Reports.for_options(opts)
    all_segments, all_scores = lab._label_scored(paths, opts, lang_id, confidence_threshold, True, reports) if paths else ([], [])
    for fi, (wav_file, segments, score) in enumerate(zip(wav_files, all_segments, all_scores)):
        print(f"\nInferencing: {wav_file}")
        lab_path = os.path.join(output_dir, os.path.splitext(wav_file)[0] + ".lab")
        _write_lab(lab_path, segments)
        _write_score(lab_path, segments, score)
        _write_reports(lab_path, reports, fi)
        print("Predicted segments:")
        for start, end, ph in segments:
            print(f"({round(start, 2)}, {round(end, 2)}, {ph})")
    def write_folder(stem, text, what):
        _write_text(os.path.join(output_dir, f"{stem}.tsv" if world == 1 else f"{stem}.rank{rank}.tsv"), text, what)

    def write_folder_reports(keys):
        for key in keys:
            if key in reports.rows:
                write_folder(R.KINDS[key].stem, R.folder_text(key, reports.named(key, wav_files)), R.KINDS[key].what + " of the folder")

    first = ("edits", "insertions")                       # draft_moves.tsv keeps its place between these two kinds and the later ones

    if opts.align_scores or opts.duration_scores or opts.optional_scores or opts.filler_scores or opts.duration_prior_scores:
        write_folder("alignment_scores", format_review_tsv([(f, sc) for f, sc in zip(wav_files, all_scores) if isinstance(sc, AL.FileScore)]),
                     "Review list")
    write_folder_reports(first)
    if opts.align_draft:
        write_folder("draft_moves", format_draft_moves_tsv([(wav_files[fi], reports.moves[fi]) for fi in sorted(reports.moves)]),
                     "Draft moves")
    write_folder_reports([key for key in R.KINDS if key not in first])
    if opts.free_scores:
        write_folder("decode_scores", format_decode_review_tsv([(f, sc) for f, sc in zip(wav_files, all_scores) if isinstance(sc, DC.FreeScore)]),
                     "Decode review list")
    return all_segments


def main(argv=None):
    import click
    from pathlib import Path

    @click.command(help="Infer with WFL")
    @click.argument("path", metavar="PATH")
    @click.option("--checkpoint", "-ckpt", type=str, required=True, help="Path to WFL Checkpoint.")
    @click.option("--config", "-c", type=str, required=True, help="Path to Config file.")
    @click.option("--output", "-o", type=str, required=False, default=".", help="Path to output labels.")
    @click.option("--lang-id", "-l", type=int, required=False, default=None, help="Language ID.")
    @click.option("--sample", "-s", is_flag=True, help="Enable sampling instead of argmax")
    @click.option("--top-k", "-tk", type=int, default=0, help="Top-K sampling (range: 1-20)")
    @click.option("--top-p", "-tp", type=float, default=0.0, help="Top-P sampling (range: 0.1-1)")
    @click.option("--temperature", "-temp", type=float, default=1.0, help="Sampling temperature (range: 0.1-2)")
    @click.option("--device", "-d", type=str, default="auto", help='Device to use: "cuda", "cuda:0". Auto-detects if not specified.')
    @click.option("--confidence-threshold", "-ct", type=float, default=None,
                  help="Suppress predictions with low confidence. Set 0 to disable.")
    @click.option("--align", "-a", type=click.Choice(ALIGN_MODES), default=None,
                  help="How a {audio}.txt transcript is aligned: greedy (string match) or viterbi (search over the logits, GPU). "
                       "Default: config postprocess.align, else greedy.")
    @click.option("--align-scores", "align_scores", is_flag=True, default=None,
                  help="With viterbi: also write {stem}.scores.tsv beside each aligned .lab (per-token posteriors by forward-backward "
                       "on the GPU) and, for a folder, alignment_scores.tsv. Default: config postprocess.align_scores, else off.")
    @click.option("--decode", "-dec", type=click.Choice(DECODE_MODES), default=None,
                  help="How files are decoded freely (no transcript, or one under --align greedy): argmax (per-frame argmax and median "
                       "filter) or viterbi (BIO-grammar search over the logits, GPU). Default: config postprocess.decode, else argmax.")
    @click.option("--switch-penalty", "switch_penalty", type=float, default=None,
                  help="With --decode viterbi: cost of every opened run, in nats (>= 0). Default: config postprocess.switch_penalty, "
                       "else 0.")
    @click.option("--decode-scores", "decode_scores", is_flag=True, default=None,
                  help="With --decode viterbi: also write {stem}.decode_scores.tsv beside each searched .lab (per-run posteriors by "
                       "forward-backward over the grammar on the GPU) and, for a folder, decode_scores.tsv. Default: config "
                       "postprocess.decode_scores, else off.")
    @click.option("--phoneme-bigram", "phoneme_bigram", type=str, default=None,
                  help="With --decode viterbi: a phoneme_bigram.json (python -m wfl_asr_amd.phonotactics); every opened run then costs "
                       "bigram_weight * log P(symbol | previous symbol) - switch_penalty. Default: config postprocess.phoneme_bigram, "
                       "else none.")
    @click.option("--bigram-weight", "bigram_weight", type=float, default=None,
                  help="With --phoneme-bigram: the weight of the bigram's log probabilities (>= 0). Default: config "
                       "postprocess.bigram_weight, else 1.")
    @click.option("--bigram-scores", "bigram_scores", is_flag=True, default=None,
                  help="With --phoneme-bigram: --decode-scores for the bigram decode; the same {stem}.decode_scores.tsv and "
                       "decode_scores.tsv, from a forward-backward pass over the grammar with the bigram's table on the GPU. Default: "
                       "config postprocess.bigram_scores, else off.")
    @click.option("--align-draft", "align_draft", type=str, default=None,
                  help="With --align viterbi: a folder of draft .lab files (X.wav -> DIR/X.lab). A file with a draft is aligned to the "
                       "draft's labels, every token opening within --draft-tolerance of its draft start; for a folder also "
                       "draft_moves.tsv. Default: config postprocess.align_draft, else none.")
    @click.option("--draft-tolerance", "draft_tolerance", type=float, default=None,
                  help="With --align-draft: seconds either side of a draft start in which the token may open (>= 0; 0 pins the "
                       "frame). Default: config postprocess.draft_tolerance, else 0.1.")
    @click.option("--align-edits", "align_edits", is_flag=True, default=None,
                  help="With --align viterbi: also write {stem}.edits.tsv beside each aligned .lab (per token the best substitute "
                       "phonemes and the deletion, as log likelihood ratios against the transcript as written, summed over all "
                       "boundaries on the GPU) and, for a folder, transcript_edits.tsv with every token an edit would improve. "
                       "Default: config postprocess.align_edits, else off.")
    @click.option("--align-insertions", "align_insertions", is_flag=True, default=None,
                  help="With --align viterbi: also write {stem}.insertions.tsv beside each aligned .lab (per place of the transcript "
                       "the best phonemes to insert there, as log likelihood ratios against the transcript as written, summed over "
                       "all boundaries on the GPU) and, for a folder, transcript_insertions.tsv with every place a token seems to be "
                       "missing. Default: config postprocess.align_insertions, else off.")
    @click.option("--min-duration", "min_duration", type=str, multiple=True,
                  help="With --align viterbi: the least time a transcript token occupies, SECONDS for every token or NAME=SECONDS for "
                       "the tokens of that name (repeatable; a plain SECONDS beside named ones is their default). At most 0.16 s "
                       "(8 frames). Default: config postprocess.min_duration, else none.")
    @click.option("--duration-scores", "duration_scores", is_flag=True, default=None,
                  help="With --min-duration: --align-scores for the alignment under minimum durations; the same {stem}.scores.tsv "
                       "and alignment_scores.tsv, from a forward-backward pass over the minimum-duration lattice on the GPU. Default: "
                       "config postprocess.duration_scores, else off.")
    @click.option("--optional", "optional_tokens", type=str, multiple=True,
                  help="With --align viterbi: a transcript token name the alignment may leave out where the audio does not hold it "
                       "(repeatable; '*' for every token), at most one between two kept tokens. The .lab lacks the skipped tokens; "
                       "{stem}.skipped.tsv and, for a folder, skipped_tokens.tsv list them. Default: config "
                       "postprocess.optional_tokens, else none.")
    @click.option("--skip-penalty", "skip_penalty", type=float, default=None,
                  help="With --optional: what a path pays per skipped token, in nats (>= 0). Default: config postprocess.skip_penalty, "
                       "else 0.")
    @click.option("--optional-scores", "optional_scores", is_flag=True, default=None,
                  help="With --optional: --align-scores for that alignment, from a forward-backward pass over the skip lattice on the "
                       "GPU: {stem}.scores.tsv for the kept tokens and {stem}.optional.tsv, per optional token whether it was kept, "
                       "the posterior probability that it is present and a doubt flag; for a folder also alignment_scores.tsv and "
                       "optional_scores.tsv, the least confident decision first. Default: config postprocess.optional_scores, else "
                       "off.")
    @click.option("--filler-token", "filler_token", type=str, default=None,
                  help="With --align viterbi: a transcript token of this name is a filler -- it stands for a stretch of audio the "
                       "transcript does not spell and matches anything, every frame at the frame's best class minus "
                       "--filler-penalty. In the .lab its span holds what the free decode found there; {stem}.fillers.tsv and, for "
                       "a folder, filler_spans.tsv list the spans. Default: config postprocess.filler_token, else none.")
    @click.option("--filler-penalty", "filler_penalty", type=float, default=None,
                  help="With --filler-token: what a filler pays per frame of its run, in nats (>= 0). Default: config "
                       "postprocess.filler_penalty, else 1.0 (a value to start from, not a measured optimum).")
    @click.option("--filler-scores", "filler_scores", is_flag=True, default=None,
                  help="With --filler-token: --align-scores for that alignment, from a forward-backward pass over the filler lattice "
                       "on the GPU: {stem}.scores.tsv, one row per transcript token, and {stem}.filler_scores.tsv, per filler the "
                       "posterior that its span belongs to it and the mean shift and spread of its start and of its end; for a "
                       "folder also alignment_scores.tsv and filler_scores.tsv, the lowest posterior first. Default: config "
                       "postprocess.filler_scores, else off.")
    @click.option("--duration-prior", "duration_prior", type=str, default=None,
                  help="With --align viterbi: a phoneme_durations.json (python -m wfl_asr_amd.durations); a run of d frames of a "
                       "transcript token then adds duration_prior_weight * log P(d | phoneme) to the path's score, in an "
                       "explicit-duration search on the GPU. Default: config postprocess.duration_prior, else none.")
    @click.option("--duration-prior-weight", "duration_prior_weight", type=float, default=None,
                  help="With --duration-prior: what the prior's log probabilities are multiplied by (>= 0). Default: config "
                       "postprocess.duration_prior_weight, else 1.0 (a value to start from, not a measured optimum).")
    @click.option("--duration-prior-scores", "duration_prior_scores", is_flag=True, default=None,
                  help="With --duration-prior: score every aligned file by a forward-backward pass over the explicit-duration "
                       "lattice of its search on the GPU: {stem}.scores.tsv, one row per transcript token, and {stem}.durations.tsv, "
                       "per token its length, the prior's log probability of it, the posterior of its run, the shift and spread "
                       "of both its ends and its expected length; for a folder also alignment_scores.tsv and token_durations.tsv, "
                       "the least probable length first. Default: config postprocess.duration_prior_scores, else off.")
    @click.option("--decode-duration-prior", "decode_duration_prior", type=str, default=None,
                  help="With --decode viterbi: a phoneme_durations.json (python -m wfl_asr_amd.durations) for the free decode; a run of "
                       "d frames of a phoneme then adds decode_duration_prior_weight * log P(d | phoneme) to the path's score, in an "
                       "explicit-duration search on the GPU (under the --phoneme-bigram table where one is given, else the flat "
                       "switch penalty). Default: config postprocess.decode_duration_prior, else none.")
    @click.option("--decode-duration-prior-weight", "decode_duration_prior_weight", type=float, default=None,
                  help="With --decode-duration-prior: what the prior's log probabilities are multiplied by (>= 0). Default: config "
                       "postprocess.decode_duration_prior_weight, else 1.0 (a value to start from, not a measured optimum).")
    @click.option("--decode-duration-scores", "decode_duration_scores", is_flag=True, default=None,
                  help="With --decode-duration-prior: --decode-scores for the duration-prior decode; the same {stem}.decode_scores.tsv "
                       "and decode_scores.tsv, from a semi-Markov forward-backward pass over the grammar with the search's tables on "
                       "the GPU. Default: config postprocess.decode_duration_scores, else off.")
    @click.option("--transcript-variants", "transcript_variants", is_flag=True, default=None,
                  help="With --align viterbi: '(', '|' and ')' in a {audio}.txt are syntax, 'k a ( t | d ) o ( N | )': 2 to 4 spellings "
                       "of a stretch, the first the transcript as written, an empty one making it optional. The search chooses among "
                       "them jointly on the GPU; {stem}.variants.tsv lists every group's choice and, for a folder, "
                       "transcript_variants.tsv the choices that are not as written. Default: config "
                       "postprocess.transcript_variants, else off.")
    def cli(path, checkpoint, config, output, lang_id, sample, top_k, top_p, temperature, device, confidence_threshold, align,
            align_scores, decode, switch_penalty, decode_scores, phoneme_bigram, bigram_weight, bigram_scores, align_draft,
            draft_tolerance, align_edits, align_insertions, min_duration, duration_scores, optional_tokens, skip_penalty,
            optional_scores, filler_token, filler_penalty, filler_scores, duration_prior, duration_prior_weight,
            duration_prior_scores, decode_duration_prior, decode_duration_prior_weight, decode_duration_scores, transcript_variants):
        if switch_penalty is not None and not switch_penalty >= 0.0:
            raise click.UsageError("--switch-penalty must be >= 0 (nats)")
        if sample:
            if top_k <= 0 and top_p <= 0.0:
                print("Sampling is enabled but neither --top-k nor --top-p is set.")
                sys.exit(1)
            if top_k > 0 and top_p > 0.0:
                print("You can't use both --top-k and --top-p at the same time.")
                sys.exit(1)
            if top_k < 0:
                print("top-k must be ≥ 1.")
                sys.exit(1)
            if top_p < 0.0 or top_p > 1.0:
                print("top-p must be between 0.1 and 1.0.")
                sys.exit(1)
            if temperature <= 0.0:
                print("temperature must be greater than 0.")
                sys.exit(1)
        requested = device.lower()
        if requested == "auto":
            device = "cuda"
        if not str(device).startswith("cuda") or not torch.cuda.is_available():
            print("This build runs on MI355X only (no CPU fallback): no ROCm device is available.", file=sys.stderr)
            sys.exit(1)
        inf_path = Path(path)
        cfg = load_config(Path(config))
        if confidence_threshold is None:
            confidence_threshold = cfg["postprocess"].get("confidence_threshold", 0.0)
        try:
            opts = resolve(cfg["postprocess"], align=align, align_scores=align_scores, decode=decode, switch_penalty=switch_penalty,
                           decode_scores=decode_scores, phoneme_bigram=phoneme_bigram, bigram_weight=bigram_weight,
                           bigram_scores=bigram_scores, align_draft=align_draft, draft_tolerance=draft_tolerance,
                           align_edits=align_edits, align_insertions=align_insertions,
                           min_duration=parse_min_duration(min_duration), duration_scores=duration_scores,
                           optional_tokens=list(optional_tokens) or None, skip_penalty=skip_penalty, optional_scores=optional_scores,
                           filler_token=filler_token, filler_penalty=filler_penalty, filler_scores=filler_scores,
                           duration_prior=duration_prior, duration_prior_weight=duration_prior_weight,
                           duration_prior_scores=duration_prior_scores, decode_duration_prior=decode_duration_prior,
                           decode_duration_prior_weight=decode_duration_prior_weight,
                           decode_duration_scores=decode_duration_scores, transcript_variants=transcript_variants)
        except ValueError as err:
            raise click.UsageError(str(err))
        output_path = inf_path if output == "." else output
        if not inf_path.exists():
            print(f"Unable to locate folder {str(inf_path)}")
            sys.exit(1)
        if lang_id is not None and lang_id <= -1:
            lang_id = None
        kw = dict(config_path=str(config), checkpoint_path=str(checkpoint), device=device, lang_id=lang_id, sample=sample,
                  top_k=top_k, top_p=top_p, temperature=temperature, confidence_threshold=confidence_threshold, align=opts.align,
                  align_scores=opts.align_scores, decode=opts.decode, switch_penalty=opts.switch_penalty,
                  decode_scores=opts.decode_scores, bigram_scores=opts.bigram_scores,
                  # an argument that is given wins over the config, so "no bigram" travels as an empty path, and a weight only beside
                  # the search it belongs to (with another decode none was given, or resolve had refused it)
                  phoneme_bigram=opts.phoneme_bigram or "",
                  bigram_weight=opts.bigram_weight if opts.decode == "viterbi" else None,
                  # the draft travels the same way: an empty path for "none", a tolerance only beside a draft
                  align_draft=opts.align_draft or "", draft_tolerance=opts.draft_tolerance if opts.align_draft else None,
                  align_edits=opts.align_edits, align_insertions=opts.align_insertions, min_duration=opts.min_duration,
                  duration_scores=opts.duration_scores,
                  # a penalty only beside the tokens it prices (with none, none was given, or resolve had refused it)
                  optional_tokens=opts.optional_tokens, skip_penalty=opts.skip_penalty if opts.optional_tokens is not None else None,
                  optional_scores=opts.optional_scores,
                  filler_token=opts.filler_token, filler_penalty=opts.filler_penalty if opts.filler_token is not None else None,
                  filler_scores=opts.filler_scores,
                  # the prior travels as the bigram does: an empty path for "none", a weight only beside a prior
                  duration_prior=opts.duration_prior or "",
                  duration_prior_weight=opts.duration_prior_weight if opts.duration_prior else None,
                  duration_prior_scores=opts.duration_prior_scores,
                  decode_duration_prior=opts.decode_duration_prior or "",
                  decode_duration_prior_weight=opts.decode_duration_prior_weight if opts.decode_duration_prior else None,
                  decode_duration_scores=opts.decode_duration_scores, transcript_variants=opts.transcript_variants)
        if inf_path.is_dir():
            infer_folder(folder_path=str(inf_path), output_dir=str(output_path), **kw)
        else:
            segments = infer_audio(audio_path=str(inf_path), output_lab_path=str(output_path), **kw)
            print("Predicted segments:")
            for start, end, ph in segments:
                print(f"({round(start, 2)}, {round(end, 2)}, {ph})")

    cli.main(args=argv, standalone_mode=True)


if __name__ == "__main__":
    main()
