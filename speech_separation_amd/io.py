"""Callers and data formats either side of the hot path: embedding / tensor loading, batch
collation with pinned staging + asynchronous H2D, and the per-item prediction writer.

Mirrors (does not import) the reference's formats and semantics:
  * ``load_object``        src/datasets/base_dataset.py:188-205   .npy / .npz (first array; make_embeddings.py:69 writes
                                                                   ``np.savez_compressed(embedding=(512,50) f32)``) / .pt|.pth,
                                                                   returned with a leading batch dim of 1
  * ``collate``            src/datasets/collate.py:4-46           tensors concatenated on dim 0, ``audio_path`` as a list,
                                                                   a key whose first item is None stays None
  * ``save_predictions``   src/trainer/inferencer.py:128-147      one ``<stem>.pth`` per item holding 1-D tensors
                                                                   {s1_pred, s2_pred[, s1_true, s2_true]}
Once the forward runs at hundreds of mixtures per second these become the bottleneck of an evaluation, so the batch is
assembled directly in reusable PINNED host buffers (one non-blocking copy per tensor, on a side stream, overlapped with
the previous batch's forward) and the predictions come back in ONE device->host copy per tensor instead of 4·B clones.
"""
from __future__ import annotations

import os
from pathlib import Path
from typing import Dict, List, Mapping, Optional, Sequence

import numpy as np
import torch

TENSOR_KEYS = ["mix_spectrogram", "complex_spectrogram", "s1_spectrogram", "s2_spectrogram", "s1_video", "s2_video",
               "s1_embedding", "s2_embedding", "mix", "s1", "s2"]
LIST_KEYS = ["audio_path"]
VIDEO_KEYS = ["s1_video", "s2_video"]


def load_object(path: str) -> torch.Tensor:
    if path.endswith(".npy"):
        obj = torch.from_numpy(np.load(path))
    elif path.endswith(".npz"):
        with np.load(path) as data:
            obj = torch.from_numpy(data[next(iter(data))])
    elif path.endswith((".pt", ".pth")):
        obj = torch.load(path)
    else:
        raise ValueError(f"unsupported object file: {path}")
    return obj.unsqueeze(0)


def load_video(path: str) -> torch.Tensor:
    """(1, Tv, H, W) float32: the ``data`` array of a mouth-crop .npz, as BaseDataset.load_video reads it
    (base_dataset.py:151-153)."""
    with np.load(path) as data:
        return torch.from_numpy(np.asarray(data["data"], dtype=np.float32)).unsqueeze(0)


def collate(items: Sequence[Mapping[str, object]]) -> Dict[str, object]:
    batch: Dict[str, object] = {}
    for key in TENSOR_KEYS + LIST_KEYS:
        if key not in items[0]:
            continue
        if items[0][key] is None:
            batch[key] = None
            continue
        vals = [it[key] for it in items]
        batch[key] = torch.cat(vals, dim=0) if key in TENSOR_KEYS else vals
    return batch


def resample(wave: torch.Tensor, orig_sr: int, new_sr: int, lowpass_filter_width: int = 6, rolloff: float = 0.99) -> torch.Tensor:
    """Band-limited sample-rate conversion of (..., T) float32 waveforms on the CPU: a restatement of what the reference's
    ``torchaudio.functional.resample(audio, sr, target_sr)`` (base_dataset.py:142-148) computes with its defaults --
    windowed-sinc interpolation (Hann window, 6 zero crossings, cut-off at 0.99 of the lower Nyquist) applied as one strided
    convolution with `new_sr / gcd` polyphase kernels; output length ceil(T * new_sr / orig_sr).
    The kernels are formed in the WAVEFORM's dtype, as torchaudio does (it passes `waveform.dtype` to its kernel builder: for
    the float32 audio the reference loads, idx, t, window and kernel are all float32) -- ADVICE r3.
    torchaudio is a third-party dependency that is not installed here and the reference holds no fixture for it: PARITY
    UNPINNED (properties only: tests/test_io.py)."""
    import math
    if orig_sr <= 0 or new_sr <= 0:
        raise ValueError("sample rates must be positive")
    if orig_sr == new_sr:
        return wave
    g = math.gcd(int(orig_sr), int(new_sr))
    orig, new = int(orig_sr) // g, int(new_sr) // g
    base = min(orig, new) * rolloff
    width = int(math.ceil(lowpass_filter_width * orig / base))
    kdt = wave.dtype if wave.dtype in (torch.float32, torch.float64) else torch.float32
    idx = torch.arange(-width, width + orig, dtype=kdt) / orig
    t = torch.arange(0, -new, -1, dtype=kdt)[:, None] / new + idx[None, :]
    t = (t * base).clamp_(-lowpass_filter_width, lowpass_filter_width)
    window = torch.cos(t * math.pi / lowpass_filter_width / 2) ** 2
    t = t * math.pi
    kernels = torch.where(t == 0, torch.ones_like(t), torch.sin(t) / t) * window * (base / orig)      # (new, 2 width + orig)
    shape, T = wave.shape[:-1], wave.shape[-1]
    x = torch.nn.functional.pad(wave.reshape(-1, 1, T).to(kdt), (width, width + orig))
    y = torch.nn.functional.conv1d(x, kernels[:, None, :], stride=orig)                             # (n, new, frames)
    y = y.transpose(1, 2).reshape(y.shape[0], -1)[:, :int(math.ceil(new * T / orig))]
    return y.reshape(*shape, y.shape[-1])


def load_audio(path: str, target_sr: Optional[int] = None) -> torch.Tensor:
    """(1, T) float32 in [-1, 1): first channel of a PCM WAV file, as BaseDataset.load_audio returns it
    (base_dataset.py:137-148; torchaudio.load normalises integer PCM by 2^(bits-1)), converted to `target_sr` when the
    file's rate differs (`resample`)."""
    import wave
    with wave.open(path, "rb") as w:
        sr, nch, width, n = w.getframerate(), w.getnchannels(), w.getsampwidth(), w.getnframes()
        raw = w.readframes(n)
    if width == 2:
        x = np.frombuffer(raw, dtype="<i2").astype(np.float32) / 32768.0
    elif width == 4:
        x = (np.frombuffer(raw, dtype="<i4").astype(np.float64) / 2147483648.0).astype(np.float32)
    else:
        raise ValueError(f"{path}: unsupported PCM sample width {width}")
    audio = torch.from_numpy(np.ascontiguousarray(x.reshape(-1, nch)[:, 0])).unsqueeze(0)
    if target_sr is not None and sr != target_sr:
        audio = resample(audio, sr, target_sr)
    return audio


def load_item(entry: Mapping[str, Optional[str]], target_sr: Optional[int] = None) -> Dict[str, object]:
    """One dataset element from its index entry, the parts of BaseDataset.__getitem__ (base_dataset.py:56-135) this path
    consumes: mix / s1 / s2 waveforms, the two lip embeddings, audio_path, and -- only for an entry that names them with
    s1_video_path / s2_video_path -- the two mouth videos (load_video).  Spectrogram keys are not produced (the
    separator ignores them, dptn_wav.py:171): spectral.add_spectrogram_keys computes them for a whole batch on the device."""
    g = lambda k: entry.get(k)
    item: Dict[str, object] = {"mix": load_audio(entry["mix_wav_path"], target_sr), "s1": None, "s2": None, "s1_video": None,
                               "s2_video": None, "s1_embedding": None, "s2_embedding": None,
                               "audio_path": entry["mix_wav_path"]}
    if g("s1_wav_path") is not None:
        item["s1"], item["s2"] = load_audio(entry["s1_wav_path"], target_sr), load_audio(entry["s2_wav_path"], target_sr)
    if g("s1_embedding_path") is not None:
        item["s1_embedding"], item["s2_embedding"] = load_object(entry["s1_embedding_path"]), load_object(entry["s2_embedding_path"])
    if g("s1_video_path") is not None:
        item["s1_video"], item["s2_video"] = load_video(entry["s1_video_path"]), load_video(entry["s2_video_path"])
    return item


class PinnedBatcher:
    """collate() into reusable pinned buffers + non-blocking H2D on a side stream.

    ``to_device(items)`` returns the batch dict with device tensors; the copies are ordered before later work on the
    CURRENT stream by an event, so the caller can use the tensors as usual.  Stream-ordering rules it keeps:
      * the device tensors are allocated on the side stream and handed to the caller's stream with ``record_stream``, so
        the caching allocator does not give their memory to the next batch's copy while a forward still reads them;
      * the pinned staging buffers are a ring of ``depth`` sets, each guarded by an event recorded after its H2D copies:
        a set is rewritten only after the copies that last read it have finished."""

    def __init__(self, device, device_tensors: Sequence[str] = ("mix", "s1", "s2", "s1_embedding", "s2_embedding"),
                 depth: int = 2):
        self.device = torch.device(device)
        self.device_tensors = list(device_tensors)
        cuda = self.device.type == "cuda"
        self._sets: List[Dict[str, torch.Tensor]] = [dict() for _ in range(max(1, depth) if cuda else 1)]
        self._events: List[Optional["torch.cuda.Event"]] = [None] * len(self._sets)
        self._turn = 0
        self._stream = torch.cuda.Stream(self.device) if cuda else None

    def _stage(self, pinned: Dict[str, torch.Tensor], key: str, vals: List[torch.Tensor]) -> torch.Tensor:
        shape = (sum(v.shape[0] for v in vals),) + tuple(vals[0].shape[1:])
        buf = pinned.get(key)
        if buf is None or tuple(buf.shape) != shape or buf.dtype != vals[0].dtype:
            buf = torch.empty(shape, dtype=vals[0].dtype, pin_memory=self.device.type == "cuda")
            pinned[key] = buf
        # the concatenation itself, written straight into pinned memory by ONE operator call (one GIL hand-over per key instead of
        # one per item: the loop runs beside a dozen loader threads)
        torch.cat(vals, dim=0, out=buf)
        return buf

    def to_device(self, items: Sequence[Mapping[str, object]]) -> Dict[str, object]:
        batch: Dict[str, object] = {}
        staged = {}
        i = self._turn
        self._turn = (i + 1) % len(self._sets)
        if self._events[i] is not None:
            self._events[i].synchronize()    # the H2D copies that last read this pinned set are done
        for key in TENSOR_KEYS + LIST_KEYS:
            if key not in items[0]:
                continue
            if items[0][key] is None:
                batch[key] = None
            elif key in LIST_KEYS:
                batch[key] = [it[key] for it in items]
            elif key in self.device_tensors or key in VIDEO_KEYS:    # videos an entry opted into go where the model runs
                staged[key] = self._stage(self._sets[i], key, [it[key] for it in items])
            else:
                batch[key] = torch.cat([it[key] for it in items], dim=0)
        if self._stream is None:
            batch.update({k: v.clone() for k, v in staged.items()})
            return batch
        cur = torch.cuda.current_stream(self.device)
        with torch.cuda.stream(self._stream):
            for k, v in staged.items():
                batch[k] = v.to(self.device, non_blocking=True)
                batch[k].record_stream(cur)
            ev = torch.cuda.Event()
            ev.record(self._stream)
        self._events[i] = ev
        cur.wait_event(ev)
        return batch


def save_predictions(batch: Mapping[str, object], out_dir: str) -> List[str]:
    """Write ``<stem>.pth`` per item (inferencer.py:128-147 format).  One D2H copy per tensor, not per item."""
    os.makedirs(out_dir, exist_ok=True)
    host = {k: batch[k].detach().to("cpu") for k in ("s1_pred", "s2_pred")}
    if batch.get("s1") is not None:
        host["s1_true"] = batch["s1"].detach().to("cpu")
        host["s2_true"] = batch["s2"].detach().to("cpu")
    paths = []
    for i, ap in enumerate(batch["audio_path"]):
        p = os.path.join(out_dir, f"{Path(ap).stem}.pth")
        torch.save({k: v[i].clone() for k, v in host.items()}, p)
        paths.append(p)
    return paths


class PredictionWriter:
    """Asynchronous form of save_predictions for a running evaluation: ``submit(batch, out_dir)`` starts the
    device->host copies on a side stream into pinned buffers and returns at once; a worker thread waits for them and
    writes the ``<stem>.pth`` files (same layout).  ``close()`` drains the queue and returns the paths written."""

    def __init__(self, device, depth: int = 3):
        import queue
        import threading
        self.device = torch.device(device)
        self._stream = torch.cuda.Stream(self.device)
        self._q: "queue.Queue" = queue.Queue(maxsize=depth)
        self._paths: List[str] = []
        self._error: Optional[BaseException] = None
        self._free: "queue.Queue" = queue.Queue()
        for _ in range(depth + 1):
            self._free.put({})
        self._thread = threading.Thread(target=self._run, daemon=True)
        self._thread.start()

    def _run(self):
        while True:
            job = self._q.get()
            if job is None:
                return
            ev, host, names, out_dir, pinned = job
            try:
                ev.synchronize()
                for i, ap in enumerate(names):
                    p = os.path.join(out_dir, f"{Path(ap).stem}.pth")
                    torch.save({k: v[i].clone() for k, v in host.items()}, p)
                    self._paths.append(p)
            except BaseException as e:      # surfaced by close()
                self._error = e
            finally:
                self._free.put(pinned)

    def submit(self, batch: Mapping[str, object], out_dir: str) -> None:
        os.makedirs(out_dir, exist_ok=True)
        src = {"s1_pred": batch["s1_pred"], "s2_pred": batch["s2_pred"]}
        if batch.get("s1") is not None:
            src["s1_true"], src["s2_true"] = batch["s1"], batch["s2"]
        pinned = self._free.get()            # a pinned set no copy is writing and no file write is reading
        cur = torch.cuda.current_stream(self.device)
        self._stream.wait_stream(cur)        # the predictions are produced on the caller's stream
        host = {}
        with torch.cuda.stream(self._stream):
            for k, v in src.items():
                buf = pinned.get(k)
                if buf is None or buf.shape != v.shape:
                    buf = torch.empty(v.shape, dtype=v.dtype, pin_memory=True)
                    pinned[k] = buf
                buf.copy_(v.detach(), non_blocking=True)
                v.record_stream(self._stream)
                host[k] = buf
            ev = torch.cuda.Event()
            ev.record(self._stream)
        self._q.put((ev, host, list(batch["audio_path"]), out_dir, pinned))

    def close(self) -> List[str]:
        self._q.put(None)
        self._thread.join()
        if self._error is not None:
            raise self._error
        return self._paths


# ---- the inverse of the loaders: a dataset in the reference's on-disk formats (bench.py's end-to-end leg, tests) ----------------
def write_wav(path: str, x, sr: int = 8000):
    """Mono PCM16 WAV of x in [-1, 1); returns the quantised samples as float32 (what load_audio reads back)."""
    import wave
    pcm = np.clip(np.round(np.asarray(x) * 32768.0), -32768, 32767).astype("<i2")
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes(pcm.tobytes())
    return pcm.astype(np.float32) / 32768.0


def write_synthetic_dataset(root: str, n: int, T: int, Tv: int = 50, emb: int = 512, sr: int = 8000, seed: int = 0):
    """n items under root/{mix,s1,s2,emb}: PCM16 WAVs of two noise sources and their sum, and the two lip embeddings as
    ``np.savez_compressed(embedding=(emb, Tv) f32)`` (make_embeddings.py:69), plus the index entries BaseDataset.__getitem__
    consumes (base_dataset.py:70-98).  Returns (entries, truth): truth holds what the loaders must read back."""
    rng = np.random.default_rng(seed)
    for d in ("mix", "s1", "s2", "emb"):
        os.makedirs(os.path.join(root, d), exist_ok=True)
    entries, truth = [], []
    for i in range(n):
        s1 = 0.1 * rng.standard_normal(T)
        s2 = 0.1 * rng.standard_normal(T)
        paths = {k: os.path.join(root, k, f"utt{i:04d}.wav") for k in ("mix", "s1", "s2")}
        q = {"s1": write_wav(paths["s1"], s1, sr), "s2": write_wav(paths["s2"], s2, sr)}
        q["mix"] = write_wav(paths["mix"], s1 + s2, sr)
        e = {}
        for k in ("s1", "s2"):
            e[k] = rng.standard_normal((emb, Tv)).astype(np.float32)
            np.savez_compressed(os.path.join(root, "emb", f"utt{i:04d}_{k}.npz"), embedding=e[k])
        entries.append({"mix_wav_path": paths["mix"], "s1_wav_path": paths["s1"], "s2_wav_path": paths["s2"],
                        "s1_video_path": None, "s2_video_path": None,
                        "s1_embedding_path": os.path.join(root, "emb", f"utt{i:04d}_s1.npz"),
                        "s2_embedding_path": os.path.join(root, "emb", f"utt{i:04d}_s2.npz")})
        truth.append({**q, "s1_embedding": e["s1"], "s2_embedding": e["s2"]})
    return entries, truth
