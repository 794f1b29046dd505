"""Input pipeline: the reference's data loaders with the per-image work moved to the GPU.

Mirrors the loader API of the reference (same function names, argument order and batch contents):
  get_all_data_loaders(conf)                       scripts/utils.py:50-156
  get_data_loader_list(root, file_list, ...)       scripts/utils.py:192-250   (ImageFilelist, scripts/data.py:25-49)
  get_data_loader_folder(input_folder, ...)        scripts/utils.py:680-740   (ImageFolder, scripts/data.py:116-153)
  get_data_loader_mask_and_im(file_list, mask_list, ...)  scripts/utils.py:638-677 (MyDataset, utils.py:270-363)
  get_synthetic_data_loader(file_list_a, file_list_b, mask_list, sem_list_a, sem_list_b, ...)
                                                   scripts/utils.py:583-635   (MyDatasetSynthetic, utils.py:458-580)
  get_fid_data_loader(file_list_a, file_list_b, ...)   scripts/utils.py:427-455 (DatasetInferenceFID, utils.py:366-424)
  default_txt_reader / default_flist_reader       scripts/utils.py:253-267 / scripts/data.py:13-23

Design (MI355X-first, not the reference's worker-process + CPU-transform pipeline):
  * host threads only DECODE files (PIL releases the GIL while decoding) into one pinned staging buffer
    per batch: [descriptors][image 0 bytes][image 1 bytes]... -> ONE async H2D copy per batch on a side stream;
  * flip / anti-aliased bilinear resize / crop / ToTensor / Normalize run as one HIP pass over the batch
    (munit_image_preprocess, munit_mask_preprocess, munit_label_preprocess: csrc/image.hip, bit-identical to PIL +
    torchvision),
    producing the channels_last fp32 batch the convolutions consume -- no per-sample CPU tensors, no
    collate, no NCHW->NHWC copy;
  * a producer thread keeps `prefetch` batches in flight, so decode + PCIe of step n+1 overlap step n;
  * data parallel: rank r takes every world_size-th sample of the epoch permutation (same seed on all ranks).
There is no CPU transform path: iterating a loader without a HIP device raises.
"""
import ctypes
import os
import queue
import random
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import _lib
from ._lib import ImageDesc

IMG_EXTENSIONS = (".jpg", ".JPG", ".jpeg", ".JPEG", ".png", ".PNG", ".ppm", ".PPM", ".bmp", ".BMP")


def default_flist_reader(flist):
    """One image path per line (scripts/data.py:13-23)."""
    with open(flist, "r") as f:
        return [line.strip() for line in f.readlines()]


def default_txt_reader(flist):
    """One whitespace-split record per line; element 0 is the path (scripts/utils.py:253-267)."""
    with open(flist, "r") as f:
        return [line.strip().split() for line in f.readlines()]


def is_image_file(filename):
    return filename.endswith(IMG_EXTENSIONS)


def make_dataset(directory):
    """All image files under `directory`, recursively (scripts/data.py:104-114)."""
    if not os.path.isdir(directory):
        raise AssertionError("%s is not a valid directory" % directory)
    images = []
    for root, _, fnames in sorted(os.walk(directory)):
        for fname in fnames:
            if is_image_file(fname):
                images.append(os.path.join(root, fname))
    return images


def resize_size(w, h, size):
    """torchvision Resize(int): shorter side -> size, other side int(size * long / short); (w, h) unchanged
    when the shorter side already matches or size is None.  Returns (rs_w, rs_h)."""
    if size is None or (w <= h and w == size) or (h <= w and h == size):
        return w, h
    if w < h:
        return size, int(size * h / w)
    return int(size * w / h), size


def shard_indices(n, batch_size, train, epoch_seed, rank=0, world_size=1):
    """Sample order of one epoch for one rank: permutation when train (shuffle=train), rank r takes
    positions r, r+world, ...; trailing samples that do not fill a batch are dropped (drop_last=True)."""
    if train:
        g = torch.Generator()
        g.manual_seed(int(epoch_seed))
        order = torch.randperm(n, generator=g).tolist()
    else:
        order = list(range(n))
    # every rank must see the same number of batches (one gradient all-reduce per step): drop the tail that
    # does not fill a global batch, then deal the rest round-robin
    nb = n // (batch_size * world_size)
    order = order[:nb * batch_size * world_size][rank::world_size]
    return [order[b * batch_size:(b + 1) * batch_size] for b in range(nb)]


def _decode_rgb(path):
    from PIL import Image
    with Image.open(path) as im:
        arr = np.asarray(im.convert("RGB"), dtype=np.uint8)
    return np.ascontiguousarray(arr)


def _decode_mask(path):
    from PIL import Image
    with Image.open(path) as im:
        if im.mode not in ("L", "P"):
            raise ValueError("munit_amd.data: mask %s has mode %r; single-band 8-bit masks (L / P) are supported"
                             % (path, im.mode))
        arr = np.frombuffer(im.tobytes(), dtype=np.uint8).reshape(im.size[1], im.size[0])
    return np.ascontiguousarray(arr)


def _decode_l(path):
    """Mask and label maps of the synthetic pairs: `.convert("L")`, as utils.py:566-568 (a `P` file goes through its
    palette here, unlike _decode_mask's raw indices)."""
    from PIL import Image
    with Image.open(path) as im:
        arr = np.asarray(im.convert("L"), dtype=np.uint8)
    return np.ascontiguousarray(arr)


# mapping() of the reference (utils.py:1356-1366) on grey values: the simulator's label colours -> class indices; every
# other grey value stays what it is.  csrc/image.hip (label_class) holds the same table.
LABEL_CLASSES = {255: 8, 200: 7, 178: 6, 149: 5, 133: 4, 76: 3, 55: 2, 29: 1, 0: 0}
LABEL_TABLE = tuple(LABEL_CLASSES.get(v, v) for v in range(256))

KIND_MASK, KIND_LABEL = 0, 1         # munit_image_desc.kind as munit_label_preprocess reads it


def _pack(groups, draws):
    """Lay out one batch for the device: [descriptors, group after group][pad to 256][payloads in the same order] (every
    payload 16-byte aligned).  groups: ordered (arrays, kind, resized) triples, every group with one array per sample or
    none at all (its descriptors stay zero); draws[b] = (flip, rs_h, rs_w, crop_i, crop_j, out_h, out_w) is shared by
    sample b's descriptors of every group; `resized` says whether a group's descriptors carry the draw's (rs_h, rs_w) or
    zeros.  Returns (descs, offsets in descriptor order, total)."""
    B = len(groups[0][0])
    descs = (ImageDesc * (len(groups) * B))()
    cur = (ctypes.sizeof(descs) + 255) // 256 * 256
    offs = []
    for g, (items, kind, resized) in enumerate(groups):
        for b, (a, dr) in enumerate(zip(items, draws)):
            flip, rs_h, rs_w, i, j, _, _ = dr
            if not resized:
                rs_h = rs_w = 0
            descs[g * B + b] = ImageDesc(cur, a.shape[0], a.shape[1], rs_h, rs_w, i, j, flip, kind)
            offs.append(cur)
            cur += (a.nbytes + 15) // 16 * 16
    return descs, offs, cur


def _image_groups(arrays, masks):
    return [(arrays, 0, True), (masks if masks is not None else (), KIND_MASK, False)]


def _synth_groups(images_a, images_b, masks, sems_a, sems_b):
    return [(images_a, 0, True), (images_b, 0, True), (masks, KIND_MASK, True), (sems_a, KIND_LABEL, True),
            (sems_b, KIND_LABEL, True)]


def pack_batch(arrays, masks, draws):
    """Lay out one batch for the device.  Layout of the staging buffer:
    [B image descs][B mask descs][pad to 256][image bytes ...][mask bytes ...] (every item 16-byte aligned); the mask
    descriptors are reserved (zero) also without masks, and munit_mask_preprocess reads no (rs_h, rs_w) from them.
    draws[b] = (flip, rs_h, rs_w, crop_i, crop_j, out_h, out_w).  Returns (descs, offsets, mask offsets, total)."""
    descs, offs, total = _pack(_image_groups(arrays, masks), draws)
    return descs, offs[:len(arrays)], offs[len(arrays):], total


def pack_synth_batch(images_a, images_b, masks, sems_a, sems_b, draws):
    """Lay out one batch of synthetic pairs for the device.  Layout of the staging buffer:
    [2B image descs: a..., b...][3B plane descs: masks..., semantic_a..., semantic_b...][pad to 256]
    [a images][b images][masks][semantic_a maps][semantic_b maps] (every item 16-byte aligned).
    draws[b] = (flip, rs_h, rs_w, crop_i, crop_j, out_h, out_w): ONE draw per sample, shared by its five descriptors;
    the planes carry the resized IMAGE's (rs_h, rs_w), which munit_label_preprocess resizes them to.
    Returns (descs, offsets in descriptor order, total)."""
    return _pack(_synth_groups(images_a, images_b, masks, sems_a, sems_b), draws)


class _StagingRing:
    """Pinned host buffers reused round-robin: hipHostMalloc of a ~20 MB batch costs milliseconds, and the producer thread
    paid it for every batch.  A slot is handed out again only after the H2D copy that read it has completed (its event)."""

    def __init__(self, slots):
        self.bufs = [None] * slots
        self.events = [None] * slots
        self.pos = 0

    def take(self, nbytes):
        k = self.pos
        self.pos = (self.pos + 1) % len(self.bufs)
        if self.events[k] is not None:
            self.events[k].synchronize()          # the copy out of this slot (issued `slots` batches ago) is done
        if self.bufs[k] is None or self.bufs[k].numel() < nbytes:
            self.bufs[k] = torch.empty(int(nbytes * 1.25), dtype=torch.uint8).pin_memory()
        return k, self.bufs[k]

    def mark(self, k, event):
        self.events[k] = event


def _lay_out(groups, n_img, draws, unequal):
    """Host half of _launch, no device needed: check the images (the first n_img groups; sample b's image of every group
    goes with draws[b]) and pack the batch.  `unequal`: the caller's message for crop sizes that differ inside the batch.
    Returns (descs, offsets, total, out_h, out_w)."""
    th, tw = draws[0][5], draws[0][6]
    for b, d in enumerate(draws):
        imgs = [items[b] for items, _, _ in groups[:n_img]]
        for x in imgs:
            if x.dtype != np.uint8 or x.ndim != 3 or x.shape[2] != 3:
                raise ValueError("images must be uint8 (H, W, 3) arrays")
        for x in imgs[1:]:                        # one draw, and so one resized size, serves all images of a sample
            if x.shape != imgs[0].shape:
                raise ValueError("the images of a synthetic pair differ in size: %s vs %s" % (imgs[0].shape[:2], x.shape[:2]))
        if (d[5], d[6]) != (th, tw):
            raise ValueError(unequal)
        if d[3] < 0 or d[4] < 0 or d[3] + th > d[1] or d[4] + tw > d[2]:
            raise ValueError("crop window (%d,%d,%d,%d) outside the resized image (%d,%d)" % (d[3], d[4], th, tw, d[1], d[2]))
    return _pack(groups, draws) + (th, tw)


def _fill(buf, descs, offs, groups):
    """Host half of _launch, second part: the descriptors and every payload into the uint8 array `buf`, nothing beyond the
    batch's `total`."""
    ctypes.memmove(buf.ctypes.data, ctypes.addressof(descs), ctypes.sizeof(descs))
    for a, o in zip([a for items, _, _ in groups for a in items], offs):
        buf[o:o + a.nbytes] = a.reshape(-1)     # a large contiguous copy: numpy drops the GIL for it


def _launch(groups, n_img, draws, unequal, plane_pass, device, stream, ring):
    """Stage one packed batch (_pack's groups: n_img groups of images, then the single-band planes) in pinned memory, upload
    it with one async copy and run the device transform on `stream`: munit_image_preprocess once over all images, then
    `plane_pass` ("munit_mask_preprocess" / "munit_label_preprocess", with its *_workspace_bytes) once over all planes.
    ring: _StagingRing to take the pinned buffer from (else a fresh one).  Returns (images (n,3,h,w) channels_last, planes
    (m,1,h,w) or None, ready event, buffers to keep alive until the event)."""
    descs, offs, total, th, tw = _lay_out(groups, n_img, draws, unequal)
    lib = _lib.load()
    slot = None
    if ring is not None:
        slot, stage = ring.take(total)
    else:
        stage = torch.empty(total, dtype=torch.uint8).pin_memory()
    # The copies run HERE, in the producer thread: the decode pool's queue already holds the files of the next `ahead`
    # batches, and copies submitted behind them made every upload wait for all of that decode work (a latency bubble per
    # batch).  A few contiguous memcpys of a few MB each, with the GIL released, cost less than that wait.
    _fill(stage.numpy(), descs, offs, groups)
    n_images = n_img * len(draws)
    n_planes = len(offs) - n_images
    ksize = 3
    for a, d in zip(groups[0][0], draws):       # a sample's images are equally sized (_lay_out): its first one decides
        ksize = max(ksize, lib.munit_image_ksize(a.shape[0], d[1]), lib.munit_image_ksize(a.shape[1], d[2]))
    vp = ctypes.c_void_p
    with torch.cuda.stream(stream):
        dev = torch.empty(total, dtype=torch.uint8, device=device)
        dev.copy_(stage[:total], non_blocking=True)     # the one H2D transfer of the batch
        if slot is not None:
            copied = torch.cuda.Event()
            copied.record(stream)
            ring.mark(slot, copied)
        st = vp(stream.cuda_stream)
        base = dev.data_ptr()
        keep = (dev,) if slot is not None else (stage, dev)    # a ring slot outlives the batch by itself

        def run(name, first_desc, out, *extra):
            n = out.shape[0]
            nws = getattr(lib, name + "_workspace_bytes")(n, th, tw, *extra)
            ws = torch.empty(max(nws, 1), dtype=torch.uint8, device=device)
            rc = getattr(lib, name)(vp(base), vp(base + first_desc * ctypes.sizeof(ImageDesc)), n, th, tw, *extra,
                                    vp(out.data_ptr()), vp(ws.data_ptr()), ctypes.c_size_t(nws), st)
            if rc:
                raise RuntimeError(name + ": " + lib.munit_last_error().decode())
            return (ws,)

        images = torch.empty((n_images, 3, th, tw), device=device, dtype=torch.float32, memory_format=torch.channels_last)
        keep += run("munit_image_preprocess", 0, images, ksize)
        planes = None
        if n_planes:
            planes = torch.empty((n_planes, 1, th, tw), device=device, dtype=torch.float32)
            keep += run(plane_pass, n_images, planes)
        ev = torch.cuda.Event()
        ev.record(stream)
    return images, planes, ev, keep


def launch_transform(arrays, masks, draws, device, stream, ring=None):
    """Stage decoded uint8 images (H,W,3) [and masks (H,W)] in pinned memory, upload them with one async copy
    and run the device transform on `stream` (_launch).  Returns (outputs, ready event, buffers to keep alive until the
    event): outputs = images (B,3,h,w) channels_last, or (images, masks (B,1,h,w)).  ring: _StagingRing to take the
    pinned buffer from (else a fresh one)."""
    images, out_masks, ev, keep = _launch(_image_groups(arrays, masks), 1, draws,
                                          "crop=False needs equally sized images inside a batch", "munit_mask_preprocess",
                                          device, stream, ring)
    return (images if masks is None else (images, out_masks)), ev, keep


def _require_device():
    if not torch.cuda.is_available():
        raise RuntimeError("munit_amd.data: the transforms run on the GPU (libmunit_hip.so); no HIP device is "
                           "visible and there is no CPU fallback")


def transform_batch(arrays, masks, draws, device=None):
    """Synchronous convenience wrapper of launch_transform on the current stream's device."""
    _require_device()
    device = device or torch.device("cuda", torch.cuda.current_device())
    out, ev, keep = launch_transform(arrays, masks, draws, device, torch.cuda.current_stream(device))
    ev.synchronize()
    return out


def launch_synth_transform(images_a, images_b, masks, sems_a, sems_b, draws, device, stream, ring=None):
    """launch_transform for synthetic pairs: decoded uint8 images (H,W,3) of both domains and the three single-band
    planes (h,w) of every sample go up in one staging buffer with one async copy; munit_image_preprocess runs once over
    the 2B images and munit_label_preprocess once over the 3B planes.  Returns ((x_as, x_bs, mask_s, sem_a, sem_b),
    ready event, buffers to keep alive): the images are the two halves of one (2B,3,h,w) channels_last batch, the other
    three the thirds of one (3B,1,h,w) batch."""
    for m in list(masks) + list(sems_a) + list(sems_b):
        if m.dtype != np.uint8 or m.ndim != 2 or m.size == 0:
            raise ValueError("masks and label maps must be non-empty uint8 (H, W) arrays")
    images, planes, ev, keep = _launch(_synth_groups(images_a, images_b, masks, sems_a, sems_b), 2, draws,
                                       "every sample of a batch needs the same crop size", "munit_label_preprocess",
                                       device, stream, ring)
    B = len(draws)
    out = (images[:B], images[B:], planes[:B], planes[B:2 * B], planes[2 * B:])
    return out, ev, keep + (images, planes)


class _Dataset:
    """Indexable view used by scripts/train.py:133-143 (`loader.dataset[i]`): one transformed sample."""

    def __init__(self, loader):
        self._loader = loader

    def __len__(self):
        return len(self._loader.image_paths)

    def __getitem__(self, index):
        out = self._loader._run_batch([index], self._loader._rng)
        if self._loader.mask_paths is not None:
            return out[0][0], out[1][0]
        return out[0]


class DeviceBatchLoader:
    """Iterable of device batches: images (B,3,h,w) channels_last fp32 in [-1,1] -- and, with masks,
    (images, masks (B,1,h,w)) tuples, like DataLoader(MyDataset)."""

    def __init__(self, image_paths, mask_paths, batch_size, train, new_size, height, width, num_workers=4,
                 crop=True, device=None, seed=0, rank=None, world_size=None, prefetch=2, torch_flip=False):
        if mask_paths is not None and len(mask_paths) != len(image_paths):
            raise ValueError("image list and mask list differ in length: %d vs %d" % (len(image_paths), len(mask_paths)))
        self.image_paths = list(image_paths)
        self.mask_paths = None if mask_paths is None else list(mask_paths)
        self.batch_size = int(batch_size)
        self.train = bool(train)
        self.new_size = new_size
        self.height, self.width = int(height), int(width)
        self.crop = bool(crop)
        self.num_workers = max(1, int(num_workers))
        self.prefetch = max(1, int(prefetch))
        self.device = device
        self.seed = int(seed)
        if rank is None or world_size is None:
            import torch.distributed as dist
            on = dist.is_available() and dist.is_initialized()
            rank = dist.get_rank() if on else 0
            world_size = dist.get_world_size() if on else 1
        self.rank, self.world_size = int(rank), int(world_size)
        self.epoch = 0
        self.flip_always_drawn = bool(torch_flip)   # MyDataset flips with or without `train` (utils.py:309-312)
        self._rng = random.Random(self.seed * 1000003 + self.rank)
        self._pool = None
        self._stream = None
        self.dataset = _Dataset(self)

    def __len__(self):
        return len(self.image_paths) // (self.batch_size * self.world_size)

    # ---------------------------------------------------------------- host side of one batch
    def draw(self, src_w, src_h, rng):
        """The random draws of one sample, in the reference's order: flip, then the crop corner inside the
        resized image (RandomCrop.get_params: randint(0, h - th), randint(0, w - tw))."""
        flip = 1 if ((self.train or self.flip_always_drawn) and rng.random() < 0.5) else 0
        rs_w, rs_h = resize_size(src_w, src_h, self.new_size)
        if self.crop:
            th, tw = self.height, self.width
            if rs_h < th or rs_w < tw:
                raise ValueError("crop (%d, %d) larger than the resized image (%d, %d)" % (th, tw, rs_h, rs_w))
            i = 0 if rs_h == th else rng.randint(0, rs_h - th)
            j = 0 if rs_w == tw else rng.randint(0, rs_w - tw)
        else:
            th, tw, i, j = rs_h, rs_w, 0, 0
        return flip, rs_h, rs_w, i, j, th, tw

    def _ensure_device(self):
        _require_device()
        if self.device is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        if self._pool is None:
            self._pool = ThreadPoolExecutor(max_workers=self.num_workers)
        if self._stream is None:
            self._stream = torch.cuda.Stream(device=self.device)

    def _files_per_sample(self):
        return 2 if self.mask_paths is not None else 1

    def _submit_decodes(self, indices):
        """Hand the files of one batch to the decode threads; returns the futures (images, masks or None)."""
        futs = [self._pool.submit(_decode_rgb, self.image_paths[k]) for k in indices]
        mfuts = None
        if self.mask_paths is not None:
            mfuts = [self._pool.submit(_decode_mask, self.mask_paths[k]) for k in indices]
        return futs, mfuts

    def _finish_batch(self, futs, mfuts, rng, ring=None):
        """Collect a batch's decodes, draw its random parameters (in sample order, as the reference does per sample) and
        launch the device transform."""
        arrays = [f.result() for f in futs]
        masks = None if mfuts is None else [f.result() for f in mfuts]
        draws = [self.draw(a.shape[1], a.shape[0], rng) for a in arrays]
        return launch_transform(arrays, masks, draws, self.device, self._stream, ring)

    def _launch_batch(self, indices, rng):
        """Decode one batch with the thread pool, draw its random parameters, launch the device transform."""
        futs, mfuts = self._submit_decodes(indices)
        return self._finish_batch(futs, mfuts, rng)

    def _hand_over(self, item):
        """Make the consumer's current stream wait for a produced batch and own its buffers."""
        out, ev, keep = item
        cur = torch.cuda.current_stream(self.device)
        cur.wait_event(ev)
        for x in (out if isinstance(out, tuple) else (out,)) + keep:
            if x.is_cuda:
                x.record_stream(cur)
        return out

    def _run_batch(self, indices, rng):
        """Synchronous single batch (dataset[i])."""
        self._ensure_device()
        return self._hand_over(self._launch_batch(indices, rng))

    # ---------------------------------------------------------------- iteration
    def __iter__(self):
        self._ensure_device()
        batches = shard_indices(len(self.image_paths), self.batch_size, self.train, self.seed + self.epoch, self.rank,
                                self.world_size)
        self.epoch += 1
        rng = self._rng
        q = queue.Queue(maxsize=self.prefetch)
        stop = threading.Event()
        device = self.device

        # Decodes run AHEAD of the batch being assembled: the files of the next `ahead` batches are already with the decode
        # threads while the producer packs and uploads the current one (round 2 decoded one batch at a time, so at most
        # batch_size of the threads ever worked and every batch also paid a fresh pinned allocation: 170 images/s whatever
        # the thread count).  The draws stay in batch order, so the random stream is unchanged.
        ahead = max(2, (2 * self.num_workers) // max(1, self.batch_size * self._files_per_sample()) + 1)
        ring = _StagingRing(self.prefetch + 3)

        def produce():
            try:
                torch.cuda.set_device(device)
                from collections import deque
                pending = deque()
                it = iter(batches)
                for idx in it:
                    pending.append(self._submit_decodes(idx))
                    if len(pending) >= ahead:
                        break
                while pending:
                    if stop.is_set():
                        return
                    futs, mfuts = pending.popleft()
                    nxt = next(it, None)
                    if nxt is not None:
                        pending.append(self._submit_decodes(nxt))
                    q.put(self._finish_batch(futs, mfuts, rng, ring))
                q.put(None)
            except BaseException as e:  # surface decode / launch errors in the consumer
                q.put(e)

        t = threading.Thread(target=produce, daemon=True)
        t.start()
        try:
            while True:
                item = q.get()
                if item is None:
                    break
                if isinstance(item, BaseException):
                    raise item
                yield self._hand_over(item)
        finally:
            stop.set()
            while t.is_alive():
                try:
                    q.get(timeout=0.05)
                except queue.Empty:
                    pass


def get_data_loader_list(root, file_list, batch_size, train, new_size=None, height=256, width=256, num_workers=4,
                         crop=True, **kw):
    """List-based loader (scripts/utils.py:192-250): `file_list` holds one path per line, relative to `root`."""
    paths = [os.path.join(root, p) for p in default_flist_reader(file_list)]
    return DeviceBatchLoader(paths, None, batch_size, train, new_size, height, width, num_workers, crop, **kw)


def get_data_loader_folder(input_folder, batch_size, train, new_size=None, height=256, width=256, num_workers=4,
                           crop=True, **kw):
    """Folder-based loader (scripts/utils.py:680-740): every image under `input_folder`, sorted."""
    paths = sorted(make_dataset(input_folder))
    if not paths:
        raise RuntimeError("Found 0 images in: " + input_folder + "\nSupported image extensions are: " +
                           ",".join(IMG_EXTENSIONS))
    return DeviceBatchLoader(paths, None, batch_size, train, new_size, height, width, num_workers, crop, **kw)


def get_data_loader_mask_and_im(file_list, mask_list, batch_size, train, new_size=None, height=256, width=256,
                                num_workers=4, crop=True, **kw):
    """Image + mask loader (scripts/utils.py:638-677, MyDataset utils.py:270-363): yields (images, masks);
    with mask_list None the second element is an empty tensor, as in the reference.  MyDataset flips with
    probability 1/2 whether or not `train` is set (utils.py:309-312)."""
    paths = [rec[0] for rec in default_txt_reader(file_list)]
    mpaths = None if mask_list is None else [rec[0] for rec in default_txt_reader(mask_list)]
    loader = DeviceBatchLoader(paths, mpaths, batch_size, train, new_size, height, width, num_workers, crop,
                               torch_flip=True, **kw)
    if mpaths is None:
        return _WithEmptyMask(loader)
    return loader


class FidPairLoader:
    """Iterable of (x_a, x_b) device batches for FID evaluation: DatasetInferenceFID (scripts/utils.py:366-424) behind
    DataLoader(shuffle=False, drop_last=True) (utils.py:448-454), on a DeviceBatchLoader without crop, flip or shuffle.

    The reference's `transform` never normalises image_b: it returns `normalizer(image_a)` a second time
    (utils.py:400-401).  Under a current torchvision, where Normalize is out of place, that yields
        x_a = 2 v - 1              (v: the resized image of list a in [0, 1])
        x_b = (x_a - 0.5) / 0.5    (list a's image normalised twice; list b's image is decoded, resized and dropped)
    and this loader reproduces exactly that, x_b on the device (munit_scale: 2 x_a + (-1), the same fp32 value).  Under
    the reference's pinned torchvision 0.2.1 Normalize works in place, and both names would hold the one doubly-normalised
    tensor.  List b is read for its records only -- it must have at least as many as list a, as the reference's
    __getitem__ indexes it -- and its files are not opened."""

    def __init__(self, paths_a, paths_b, batch_size, new_size, num_workers=4, **kw):
        if len(paths_b) < len(paths_a):
            raise ValueError("FID list b has %d records, list a %d: every sample of a needs a partner" %
                             (len(paths_b), len(paths_a)))
        # the reference does not shard this loader: every process evaluates the whole list
        kw.setdefault("rank", 0)
        kw.setdefault("world_size", 1)
        self.target_paths = list(paths_b)
        self._loader = DeviceBatchLoader(paths_a, None, batch_size, False, new_size, new_size, new_size, num_workers,
                                         crop=False, **kw)
        self.image_paths = self._loader.image_paths
        self.batch_size = self._loader.batch_size

    def __len__(self):
        return len(self._loader)

    def __iter__(self):
        lib = _lib.load()
        for x_a in self._loader:
            x_b = torch.full_like(x_a, -1.0)     # same (channels_last) memory order as x_a
            with torch.cuda.device(x_a.device):
                stream = ctypes.c_void_p(torch.cuda.current_stream(x_a.device).cuda_stream)
                _lib.check(lib.munit_scale(ctypes.c_void_p(x_a.data_ptr()), ctypes.c_void_p(x_b.data_ptr()), x_a.numel(),
                                           2.0, 1, stream), "scale (FID loader)")
            yield x_a, x_b


def get_fid_data_loader(file_list_a, file_list_b, batch_size, train, new_size=256, num_workers=4, **kw):
    """FID evaluation loader (scripts/utils.py:427-455): yields (x_a, x_b), see FidPairLoader for what x_b is.  `train` is
    accepted and ignored, as in the reference (no flip, no crop, no shuffle either way)."""
    paths_a = [rec[0] for rec in default_txt_reader(file_list_a)]
    paths_b = [rec[0] for rec in default_txt_reader(file_list_b)]
    return FidPairLoader(paths_a, paths_b, batch_size, new_size, num_workers, **kw)


class _SyntheticDataset:
    """`loader.dataset[i]`: the five transformed tensors of one sample, as MyDatasetSynthetic.__getitem__ returns them."""

    def __init__(self, loader):
        self._loader = loader

    def __len__(self):
        return len(self._loader.image_paths)

    def __getitem__(self, index):
        return tuple(t[0] for t in self._loader._run_batch([index], self._loader._rng))


class SyntheticPairLoader(DeviceBatchLoader):
    """Iterable of (x_as, x_bs, mask_s, sem_a, sem_b) device batches, like DataLoader(MyDatasetSynthetic): the images
    (B,3,h,w) channels_last fp32 in [-1,1], the mask (0 / 1) and the two label maps (class indices) (B,1,h,w) fp32.
    Every sample makes ONE draw -- the flip, whatever `train` says (utils.py:496), then the crop corner inside the resized
    image_b -- shared by its five planes.  The prefetch thread, the staging ring and the sharding are the base class's."""

    def __init__(self, paths_a, paths_b, mask_paths, sem_paths_a, sem_paths_b, batch_size, train, new_size, height, width,
                 num_workers=4, device=None, seed=0, rank=None, world_size=None, prefetch=2):
        names = ("file_list_a", "file_list_b", "mask_list", "sem_list_a", "sem_list_b")
        lists = (paths_a, paths_b, mask_paths, sem_paths_a, sem_paths_b)
        if len(set(len(p) for p in lists)) != 1:
            raise ValueError("the five lists of the synthetic loader differ in length: "
                             + ", ".join("%s %d" % (n, len(p)) for n, p in zip(names, lists)))
        DeviceBatchLoader.__init__(self, paths_a, mask_paths, batch_size, train, new_size, height, width, num_workers,
                                   True, device, seed, rank, world_size, prefetch, torch_flip=True)
        self.pair_paths = list(paths_b)
        self.sem_a_paths = list(sem_paths_a)
        self.sem_b_paths = list(sem_paths_b)
        self.dataset = _SyntheticDataset(self)

    def _files_per_sample(self):
        return 5

    def sample_files(self, k):
        return (self.image_paths[k], self.pair_paths[k], self.mask_paths[k], self.sem_a_paths[k], self.sem_b_paths[k])

    def decode_sample(self, k):
        """The five decoded planes of sample k (in the calling thread)."""
        pa, pb, pm, sa, sb = self.sample_files(k)
        return _decode_rgb(pa), _decode_rgb(pb), _decode_l(pm), _decode_l(sa), _decode_l(sb)

    def draw_batch(self, indices, samples, rng):
        """Host checks and draws of one batch, in sample order; no device work.  A pair whose two images differ in size is
        refused: the reference would crop image_a with a window drawn for image_b and let PIL pad, which breaks the pixel
        alignment the pair loss is defined on."""
        draws = []
        for k, (a, b_, _, _, _) in zip(indices, samples):
            if a.shape != b_.shape:
                raise ValueError("munit_amd.data: the images of synthetic pair %d differ in size: %s is %dx%d, %s is %dx%d"
                                 % (k, self.image_paths[k], a.shape[1], a.shape[0], self.pair_paths[k], b_.shape[1],
                                    b_.shape[0]))
            draws.append(self.draw(b_.shape[1], b_.shape[0], rng))
        return draws

    def _submit_decodes(self, indices):
        futs = [[self._pool.submit(_decode_rgb if n < 2 else _decode_l, p) for n, p in enumerate(self.sample_files(k))]
                for k in indices]
        return futs, list(indices)

    def _finish_batch(self, futs, indices, rng, ring=None):
        samples = [[f.result() for f in fs] for fs in futs]
        draws = self.draw_batch(indices, samples, rng)
        cols = list(zip(*samples))
        return launch_synth_transform(cols[0], cols[1], cols[2], cols[3], cols[4], draws, self.device, self._stream, ring)


def get_synthetic_data_loader(file_list_a, file_list_b, mask_list, sem_list_a, sem_list_b, batch_size, train,
                              new_size=256, height=256, width=256, num_workers=4, crop=True, **kw):
    """Synthetic paired loader (scripts/utils.py:583-635, MyDatasetSynthetic utils.py:458-580): yields
    (x_as, x_bs, mask_s, sem_a, sem_b), what gen_update(..., synth=True, semantic_gt_a, semantic_gt_b) consumes.  Each of
    the five lists holds one record per line, element 0 the path.  `crop` is accepted and ignored, as in the reference:
    its dataset always crops.  Keyword extras: device, seed, rank, world_size, prefetch."""
    lists = [[rec[0] for rec in default_txt_reader(f)] for f in (file_list_a, file_list_b, mask_list, sem_list_a, sem_list_b)]
    return SyntheticPairLoader(lists[0], lists[1], lists[2], lists[3], lists[4], batch_size, train, new_size, height,
                               width, num_workers, **kw)


class _WithEmptyMask:
    """MyDataset without a mask list returns (image, torch.tensor([])) (utils.py:357-360)."""

    def __init__(self, loader):
        self._loader = loader
        self.dataset = loader.dataset

    def __len__(self):
        return len(self._loader)

    def __iter__(self):
        for images in self._loader:
            yield images, torch.empty((images.shape[0], 0))


def get_all_data_loaders(conf, **kw):
    """train/test loaders of both domains (scripts/utils.py:50-156): `data_root` selects the folder layout
    (trainA/testA/trainB/testB), otherwise the data_folder_* / data_list_* keys are used.  Test loaders use
    new_size for the crop as well and do not shuffle or flip."""
    batch_size = conf["batch_size"]
    num_workers = conf["num_workers"]
    if "new_size" in conf:
        new_size_a = new_size_b = conf["new_size"]
    else:
        new_size_a, new_size_b = conf["new_size_a"], conf["new_size_b"]
    height, width = conf["crop_image_height"], conf["crop_image_width"]
    out = []
    for dom, ns in (("a", new_size_a), ("b", new_size_b)):
        for train in (True, False):
            h, w = (height, width) if train else (ns, ns)
            if "data_root" in conf:
                folder = os.path.join(conf["data_root"], ("train" if train else "test") + dom.upper())
                out.append(get_data_loader_folder(folder, batch_size, train, ns, h, w, num_workers, True, **kw))
            else:
                split = "train" if train else "test"
                out.append(get_data_loader_list(conf["data_folder_%s_%s" % (split, dom)],
                                                conf["data_list_%s_%s" % (split, dom)], batch_size, train, ns, h, w,
                                                num_workers, True, **kw))
    train_a, test_a, train_b, test_b = out
    return train_a, train_b, test_a, test_b
