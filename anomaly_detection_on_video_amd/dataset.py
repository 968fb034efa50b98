"""Pre-extracted feature datasets: the `FeatureDataset` / `build_feature_dataset` surface of
`/root/reference/src/dataset.py:24-142` (zip of `<video>_i3d.npy` files, normal/abnormal split by
"Normal" in the file name, L2-magnitude channel appended per item, frame-level labels from
`ground_truth.json` in test mode).  Hub download is kept as the fallback when no `local_path` is
given (needs network); everything else works from local files, and
`write_synthetic_feature_zips` fabricates a UCF-Crime-shaped corpus for tests / benchmarks.

Video decoding + TenCrop (`TenCropVideoFrameDataset`, decord / torchvision) is outside the hot
path: extraction sources are tensors (see extract.py).
"""
from __future__ import annotations

import io
import json
import os
import zipfile
from typing import Callable, Dict, List, Optional, Union

import numpy as np
from torch.utils.data import Dataset, Sampler

DEFAULT_FEATURE_HUB = "jinmang2/ucf_crime_tencrop_i3d_seg32"
DEFAULT_FILENAMES = {"train": "train.zip", "test": "test.zip"}


class FeatureDataset(Dataset):
    def __init__(self, filenames: List[str], values: Dict[str, Union[zipfile.ZipInfo, np.ndarray]],
                 labels: Optional[Dict[str, List[float]]] = None, open_func: Optional[Callable] = None):
        self.filenames = filenames
        self.values = values
        self.labels = labels
        self.open_func = open_func

    def __len__(self) -> int:
        return len(self.values)

    def open(self, value):
        if self.open_func is None:
            return value
        return np.load(self.open_func(value))  # dynamic loading straight from the zip member

    def add_magnitude(self, feature: np.ndarray) -> np.ndarray:
        # (a, b, C) -> (a, b, C+1): append ||f||_2 (dataset.py:121-124)
        return np.concatenate((feature, np.linalg.norm(feature, axis=2)[:, :, np.newaxis]), axis=2)

    def get_filename(self, idx: int) -> str:
        return self.filenames[idx]

    def __getitem__(self, idx: int) -> Dict[str, np.ndarray]:
        fname = self.get_filename(idx)
        feature = self.open(self.values[fname])
        item = {
            "feature": self.add_magnitude(feature),
            "anomaly": np.array(0.0 if "Normal" in fname else 1.0, dtype=np.float32),
        }
        if self.labels is not None:
            key = fname if fname in self.labels else fname.replace("_i3d.npy", "")
            item["label"] = np.array(self.labels[key], dtype=np.float32)
        return item


def _build_feature_dataset(filepath: str, mode: str, dynamic_load: bool, ground_truth: Optional[Dict] = None):
    assert mode in ("train", "test")
    zipf = zipfile.ZipFile(filepath)
    filenames, values = [], {}
    for member in zipf.infolist():
        if member.is_dir():
            continue
        name = member.filename.split("/")[-1]
        filenames.append(name)
        values[name] = member if dynamic_load else np.load(zipf.open(member))
    opener = zipf.open if dynamic_load else None
    if mode == "test":
        if ground_truth is None:
            from huggingface_hub import hf_hub_download

            with open(hf_hub_download(repo_id=DEFAULT_FEATURE_HUB, filename="ground_truth.json", repo_type="dataset")) as f:
                ground_truth = json.load(f)
        return FeatureDataset(filenames=filenames, values=values, labels=ground_truth, open_func=opener)
    out = {}
    for split, pick in (("normal", lambda n: "Normal" in n), ("abnormal", lambda n: "Normal" not in n)):
        names = [n for n in filenames if pick(n)]
        out[split] = FeatureDataset(filenames=names, values={n: values[n] for n in names}, open_func=opener)
    return out


# ---------------------------------------------------------------------------------- epoch shuffling (data.shuffle)
def epoch_order(n: int, seed: int, stream: int, epoch: int, restart: int = 0) -> np.ndarray:
    """The order (int64, a permutation of range(n)) in which a class's videos are visited: a stated function of four integers,
    np.random.RandomState([seed, stream, epoch, restart]).permutation(n) -- NumPy's frozen generator, so it depends on no torch
    version and no process state, and a resumed run reproduces it.  `stream`: 0 = the normal class, 1 = the abnormal one;
    `restart`: how often that class's loader has been started again inside the epoch (Trainer._max_size_cycle restarts the shorter
    class).  Each of the four lies in [0, 2**32)."""
    for name, v in (("seed", seed), ("stream", stream), ("epoch", epoch), ("restart", restart)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) < 2 ** 32:
            raise ValueError(f"epoch_order: {name}={v!r} is outside [0, 2**32)")
    if int(n) < 0:
        raise ValueError(f"epoch_order: n={n!r} is negative")
    return np.random.RandomState([int(seed), int(stream), int(epoch), int(restart)]).permutation(int(n)).astype(np.int64, copy=False)


class ShuffledSampler(Sampler):
    """The sampler of a host DataLoader under data.shuffle: every __iter__ yields the next restart's `epoch_order`, starting at
    restart 0.  A DataLoader iterates its sampler in the main process, so the order is the same at any num_workers."""

    def __init__(self, n: int, seed: int, stream: int, epoch: int):
        epoch_order(0, seed, stream, epoch)  # (refuses bad values here, not at the first batch)
        self.n, self.seed, self.stream, self.epoch = int(n), int(seed), int(stream), int(epoch)
        self.restart = 0

    def __len__(self) -> int:
        return self.n

    def __iter__(self):
        order = epoch_order(self.n, self.seed, self.stream, self.epoch, self.restart)
        self.restart += 1
        return iter(order.tolist())


# ---------------------------------------------------------------------------------- device-resident datasets
DEFAULT_RESIDENT_MAX_BYTES = 32 << 30  # a guard against a corpus that cannot fit, not a tuned value (UCF-Crime: about 10 GB)


class ResidentFeatureDataset:
    """A feature zip held in device memory, every item as `FeatureDataset.__getitem__` returns it (magnitude channel appended,
    bit for bit: mil_ops.add_magnitude_np), so that a training step's input work is a device-to-device copy of a slice.

    Train mode (one per class, `name` = "normal" / "abnormal"): `features` (N, ncrops, seg, C+1) and `anomaly` (N,) on the device;
    item i = views of row i.  Test mode (`labels` given): `store` is one flat allocation, video i lives at floats
    [offsets[i], offsets[i+1]) TRANSPOSED, `videos[i]` = (ncrops, T, C+1) -- the layout validation_step's
    permute(0, 2, 1, 3).contiguous() asks for; item i's feature is the (T, ncrops, C+1) view of it, the label stays on the host."""

    def __init__(self, filenames: List[str], name: str = "", features=None, anomaly=None, store=None, videos=None,
                 offsets: Optional[List[int]] = None, labels: Optional[List[np.ndarray]] = None):
        self.filenames, self.name = list(filenames), name
        self.features, self.anomaly = features, anomaly
        self.store, self.videos, self.offsets, self.labels = store, videos, offsets, labels

    @property
    def nbytes(self) -> int:
        t = self.features if self.features is not None else self.store
        return int(t.numel() * t.element_size()) + (0 if self.anomaly is None else int(self.anomaly.numel() * self.anomaly.element_size()))

    def __len__(self) -> int:
        return len(self.filenames)

    def get_filename(self, idx: int) -> str:
        return self.filenames[idx]

    def __getitem__(self, idx: int):
        if not -len(self) <= idx < len(self):
            raise IndexError(idx)
        if self.videos is None:
            return {"feature": self.features[idx], "anomaly": self.anomaly[idx]}
        return {"feature": self.videos[idx].permute(1, 0, 2),
                "anomaly": np.array(0.0 if "Normal" in self.filenames[idx] else 1.0, dtype=np.float32), "label": self.labels[idx]}


class ResidentBatches:
    """DataLoader(ds, batch_size, shuffle=False, drop_last=True) over a resident train dataset: len = N // batch_size, batch i =
    {"feature": ds.features[i*B:(i+1)*B], "anomaly": ds.anomaly[i*B:(i+1)*B]} as views (nothing is copied or launched)."""

    def __init__(self, dataset, batch_size: int):
        self.dataset, self.batch_size = dataset, int(batch_size)
        if self.batch_size < 1:
            raise ValueError(f"batch_size {batch_size} must be at least 1")
        if len(dataset) < self.batch_size:
            raise ValueError(f"the {getattr(dataset, 'name', '') or 'train'} class has {len(dataset)} videos, fewer than batch_size "
                             f"{self.batch_size}: drop_last would leave no batch")

    def __len__(self) -> int:
        return len(self.dataset) // self.batch_size

    def __iter__(self):
        b = self.batch_size
        for i in range(len(self)):
            yield {"feature": self.dataset.features[i * b:(i + 1) * b], "anomaly": self.dataset.anomaly[i * b:(i + 1) * b]}


class StoreRows:
    """One class's half of a shuffled resident step: rows `rows` (a device int64 vector, a view of the loader's order table) of
    `dataset`'s store.  Trainer._feed_graph_inputs gathers a pair of them straight into the captured step's buffers
    (mil_ops.gather_batch: one launch); `materialize()` gives the ordinary batch dict, gathered with the same op into a buffer the
    loader owns (overwritten by the loader's next materialised step)."""

    def __init__(self, loader: "ShuffledResidentBatches", rows):
        self.loader, self.dataset, self.rows = loader, loader.dataset, rows

    def materialize(self) -> Dict:
        from . import mil_ops

        ds = self.dataset
        feature, anomaly = self.loader.buffers()
        mil_ops.gather_batch(ds.features, self.rows, None, None, feature, labels0=ds.anomaly, dst_labels0=anomaly)
        return {"feature": feature, "anomaly": anomaly}


class ShuffledResidentBatches(ResidentBatches):
    """ResidentBatches under data.shuffle: every __iter__ takes the next restart's epoch_order(len(dataset), seed, stream, epoch,
    restart), keeps its first len(self) * batch_size entries (what drop_last keeps) and puts them on the device once -- from pinned
    memory, non-blocking, on the current stream; no per-step upload, no synchronisation.  Step i is a `StoreRows` over the view
    [i*B, (i+1)*B) of that table (`self.table`: the last one uploaded)."""

    def __init__(self, dataset, batch_size: int, seed: int, stream: int, epoch: int):
        super().__init__(dataset, batch_size)
        epoch_order(0, seed, stream, epoch)
        self.seed, self.stream, self.epoch, self.restart = int(seed), int(stream), int(epoch), 0
        self.table = None
        self._buffers = None

    def buffers(self):
        if self._buffers is None:
            import torch

            f = self.dataset.features
            self._buffers = (torch.empty((self.batch_size,) + tuple(f.shape[1:]), dtype=f.dtype, device=f.device),
                             torch.empty((self.batch_size,), dtype=self.dataset.anomaly.dtype, device=f.device))
        return self._buffers

    def __iter__(self):
        import torch

        b, steps = self.batch_size, len(self)
        order = epoch_order(len(self.dataset), self.seed, self.stream, self.epoch, self.restart)[:steps * b]
        self.restart += 1
        # (a fresh pinned block per start: torch's host allocator hands it out again only after this copy has run)
        table = self.table = torch.from_numpy(np.ascontiguousarray(order)).pin_memory().to(self.dataset.features.device, non_blocking=True)
        return (StoreRows(self, table[i * b:(i + 1) * b]) for i in range(steps))


class ResidentItems:
    """DataLoader(ds, batch_size=1, shuffle=False) over a resident test dataset: every item with a leading 1, the feature a view
    of the store."""

    def __init__(self, dataset):
        self.dataset = dataset

    def __len__(self) -> int:
        return len(self.dataset)

    def __iter__(self):
        import torch

        for i in range(len(self.dataset)):
            item = self.dataset[i]
            yield {"feature": item["feature"].unsqueeze(0), "anomaly": torch.from_numpy(item["anomaly"].reshape(1)),
                   "label": torch.from_numpy(item["label"]).unsqueeze(0)}


def _npy_header(fp):
    """(shape, dtype) of an .npy stream, which is left at the first data byte."""
    from numpy.lib import format as npf

    version = npf.read_magic(fp)
    read = {(1, 0): npf.read_array_header_1_0, (2, 0): npf.read_array_header_2_0}.get(tuple(version))
    if read is None:
        raise ValueError(f"unsupported .npy version {version}")
    shape, fortran, dtype = read(fp)
    if fortran and len(shape) > 1:
        raise ValueError("Fortran-ordered array")
    return tuple(int(d) for d in shape), dtype


def _build_resident_dataset(filepath: str, mode: str, ground_truth: Optional[Dict], device, max_bytes: int):
    import torch

    zipf = zipfile.ZipFile(filepath)
    members = [m for m in zipf.infolist() if not m.is_dir()]
    names = [m.filename.split("/")[-1] for m in members]
    # pass 1, headers only: every shape is known, and the byte total checked, before anything is allocated
    shapes = []
    for m, name in zip(members, names):
        with zipf.open(m) as fp:
            try:
                shape, dtype = _npy_header(fp)
            except ValueError as e:
                raise ValueError(f"{name}: {e}") from e
        if dtype != np.float32 or len(shape) != 3 or 0 in shape:
            raise ValueError(f"{name}: a resident dataset holds non-empty float32 (a, b, C) features, got {dtype} {shape}")
        shapes.append(shape)
    if not members:
        raise ValueError(f"{filepath}: no features")
    if mode == "train":
        for name, shape in zip(names, shapes):
            if shape != shapes[0]:
                raise ValueError(f"{name} has shape {shape}, {names[0]} has {shapes[0]}: a resident train store needs one shape")
    elif len({s[1:] for s in shapes}) != 1:
        bad = next(i for i, s in enumerate(shapes) if s[1:] != shapes[0][1:])
        raise ValueError(f"{names[bad]} has shape {shapes[bad]}, {names[0]} has {shapes[0]}: crops and channels must agree")
    out_floats = [s[0] * s[1] * (s[2] + 1) for s in shapes]
    need = 4 * sum(out_floats) + (4 * len(members) if mode == "train" else 0)
    if need > max_bytes:
        raise ValueError(f"{filepath}: a resident {mode} dataset needs {need} bytes of device memory, above resident_max_bytes = {max_bytes}")
    if mode == "test" and ground_truth is None:
        from huggingface_hub import hf_hub_download

        with open(hf_hub_download(repo_id=DEFAULT_FEATURE_HUB, filename="ground_truth.json", repo_type="dataset")) as f:
            ground_truth = json.load(f)

    from . import mil_ops

    device = torch.device(device)
    if device.type != "cuda":
        from ._lib import HipExtensionError

        raise HipExtensionError(f"a resident dataset lives in GPU memory; got device '{device}' (there is no CPU fallback)")
    # pass 2: zip member -> pinned staging -> device staging (a, b, C) -> magnitude kernel -> its slot of the store, all on the
    # current stream.  The device staging buffer is reused in stream order; the two pinned buffers alternate, each refilled only
    # once the copy that last read it has completed (its event).  One synchronisation at the end.
    in_floats = max(s[0] * s[1] * s[2] for s in shapes)
    pinned = [torch.empty(in_floats, dtype=torch.float32).pin_memory() for _ in range(2)]
    done = [None, None]
    stage = torch.empty(in_floats, dtype=torch.float32, device=device)
    if mode == "train":
        a, b, c = shapes[0]
        order = [i for i, n in enumerate(names) if "Normal" in n] + [i for i, n in enumerate(names) if "Normal" not in n]
        n_normal = sum("Normal" in n for n in names)
        store = torch.empty((len(members), a, b, c + 1), dtype=torch.float32, device=device)
        slots = {i: store[k] for k, i in enumerate(order)}
    else:
        offsets = [0]
        for n in out_floats:
            offsets.append(offsets[-1] + n)
        store = torch.empty(offsets[-1], dtype=torch.float32, device=device)
        slots = {i: store[offsets[i]:offsets[i + 1]].view(s[1], s[0], s[2] + 1) for i, s in enumerate(shapes)}
    for i, (m, shape) in enumerate(zip(members, shapes)):
        k, n = i % 2, shape[0] * shape[1] * shape[2]
        if done[k] is not None:
            done[k].synchronize()
        with zipf.open(m) as fp:
            pinned[k].numpy()[:n] = np.load(fp).reshape(-1)
        stage[:n].copy_(pinned[k][:n], non_blocking=True)
        done[k] = torch.cuda.Event()
        done[k].record()
        mil_ops.add_magnitude_np(stage[:n].view(shape), transpose=mode == "test", out=slots[i])
    torch.cuda.current_stream(device).synchronize()
    if mode == "test":
        labels = []
        for name in names:
            key = name if name in ground_truth else name.replace("_i3d.npy", "")
            labels.append(np.array(ground_truth[key], dtype=np.float32))
        return ResidentFeatureDataset(names, "test", store=store, videos=[slots[i] for i in range(len(members))], offsets=offsets, labels=labels)
    anomaly = torch.tensor([0.0] * n_normal + [1.0] * (len(members) - n_normal), dtype=torch.float32, device=device)
    split = {"normal": slice(0, n_normal), "abnormal": slice(n_normal, len(members))}
    return {cls: ResidentFeatureDataset([names[i] for i in order[sl]], cls, features=store[sl], anomaly=anomaly[sl]) for cls, sl in split.items()}


def build_feature_dataset(mode: str = "train", local_path: Optional[str] = None, filename: Optional[str] = None,
                          cache_dir: Optional[str] = None, revision: str = "main", dynamic_load: bool = True,
                          resident=None, resident_max_bytes: int = DEFAULT_RESIDENT_MAX_BYTES):
    """Reference signature (dataset.py:73-95).  With `local_path`+`filename` the zip (and, in test
    mode, `<local_path>/ground_truth.json`) is read locally; otherwise it is fetched from the hub.
    `resident` (a GPU device; default None = the host datasets above): the whole zip is loaded once into device memory, magnitude
    channel included, and `ResidentFeatureDataset`s are returned (`dynamic_load` does not apply).  More than `resident_max_bytes`
    of device memory is refused before anything is allocated."""
    assert mode in ("train", "test")
    assert sum([local_path is None, filename is None]) != 1
    gt = None
    if local_path is None:
        from huggingface_hub import hf_hub_download

        filepath = hf_hub_download(repo_id=DEFAULT_FEATURE_HUB, filename=DEFAULT_FILENAMES[mode], cache_dir=cache_dir,
                                   revision=revision, repo_type="dataset")
    else:
        filepath = os.path.join(local_path, filename)
        gt_path = os.path.join(local_path, "ground_truth.json")
        if mode == "test" and os.path.exists(gt_path):
            with open(gt_path) as f:
                gt = json.load(f)
    if resident is not None:
        return _build_resident_dataset(filepath, mode, gt, resident, int(resident_max_bytes))
    return _build_feature_dataset(filepath, mode, dynamic_load, gt)


def write_synthetic_feature_zips(outdir: str, n_normal: int = 8, n_abnormal: int = 8, n_test: int = 6, seg: int = 32,
                                 channels: int = 2048, ncrops: int = 10, seed: int = 0) -> str:
    """A small UCF-Crime-shaped feature corpus: train.zip ((10, seg, C) per video), test.zip
    ((n_clips, 10, C) per video) and ground_truth.json built with the make_gt_ucf rule.  Abnormal
    videos carry a burst of larger-magnitude features on the annotated clips."""
    from .gt import frame_ground_truth

    rng = np.random.default_rng(seed)
    os.makedirs(outdir, exist_ok=True)

    def put(z, name, arr):
        buf = io.BytesIO()
        np.save(buf, arr.astype(np.float32))
        z.writestr(name, buf.getvalue())

    with zipfile.ZipFile(os.path.join(outdir, "train.zip"), "w") as z:
        for i in range(n_normal):
            put(z, f"train/Normal_Videos{i:03d}_x264_i3d.npy", np.abs(rng.standard_normal((ncrops, seg, channels))))
        for i in range(n_abnormal):
            f = np.abs(rng.standard_normal((ncrops, seg, channels)))
            s = int(rng.integers(0, seg - 6))
            f[:, s : s + 6] *= 2.5
            put(z, f"train/Abuse{i:03d}_x264_i3d.npy", f)
    gt = {}
    with zipfile.ZipFile(os.path.join(outdir, "test.zip"), "w") as z:
        for i in range(n_test):
            n_clips = int(rng.integers(20, 60))
            f = np.abs(rng.standard_normal((n_clips, ncrops, channels)))
            if i % 2 == 0:
                name, ev = f"Normal_Videos_{900 + i}_x264", ((-1, -1), (-1, -1))
            else:
                c0 = int(rng.integers(2, n_clips - 8))
                f[c0 : c0 + 6] *= 2.5
                name, ev = f"Burglary{i:03d}_x264", ((c0 * 16, (c0 + 6) * 16 - 1), (-1, -1))
            put(z, f"test/{name}_i3d.npy", f)
            gt[name] = frame_ground_truth(n_clips, ev[0], ev[1])
    with open(os.path.join(outdir, "ground_truth.json"), "w") as f:
        json.dump(gt, f)
    return outdir
