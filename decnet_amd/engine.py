"""Streaming inference: uint8 stereo pairs in, uint16 disparity maps out, the forward as one HIP graph per shape.

    engine = decnet_amd.StereoEngine(model, batch_size=8)
    engine.submit(lefts, rights, tag="batch 0")          # lists of h x w x 3 uint8 arrays, at most batch_size
    for tag, disps, metrics in engine.results(): ...     # what is finished, in submission order; never blocks
    engine.flush()                                       # waits for everything that was submitted

What happens to a batch (``depth`` of them are in flight, each in its own slot of pinned + device staging):

  copy stream     H2D of the uint8 views (and the ground truth)        ................  D2H of the uint16 maps
  compute stream  ............ preprocess_u8 x2 -> graph replay -> disparity_to_u16 (-> disparity_metrics) ......

ordered by events.  The D2H of batch k is put on the copy stream BEHIND the H2D of batch k + 1 (it is enqueued by the next
``submit``, by ``flush``, or by ``results`` once the batch has computed), so the upload of the next batch never waits for
the batch that computes.  The host blocks in ``submit`` when every slot is busy and in ``flush``; nothing else waits and nothing reads a scalar back.

Shape buckets: a bucket is keyed by (B, H, W, max_disp), B = batch_size (a shorter batch is filled with copies of its
last pair, whose outputs are dropped) and H x W the size padded to multiples of 27.  It owns the static input tensors, ONE
captured graph of ``model(left, right)`` under no_grad, and the graph's output.  Pre- and postprocessing are eager
launches around the replay: they take the slot's buffers and the unpadded size as arguments, which change from batch to
batch, while everything the graph reads sits at fixed addresses.  A graph also reads the model's packed weights and
workspaces at the addresses of its capture, and the model replaces those when another shape or range
needs larger or other ones: a bucket therefore keeps every cache tensor of its capture alive, so that the memory cannot be
handed out again while the graph may run.  At most ``max_buckets`` live, least recently used out first.

``reset()`` drops every bucket: REQUIRED after any weight change and after ``drop_weight_caches`` (the old graphs would
compute with the old weights).  Every HIP call is made by the thread that calls submit / results / flush / reset.
While batches are in flight nothing else may run the model: eager calls and the graphs share its workspaces.
"""
import collections

import numpy as np
import torch

from . import imageio


class _Bucket:
    """Static tensors + the captured forward of one (B, H, W, max_disp)."""

    def __init__(self, model, key, device, stream):
        B, H, W, D = key
        self.key = key
        self.last_use = None                                # event behind the last launch that touches this bucket
        saved = model.max_disp
        model.max_disp = D
        try:
            with torch.no_grad(), torch.cuda.stream(stream):
                self.left = torch.zeros((B, 3, H, W), dtype=torch.float32, device=device)
                self.right = torch.zeros((B, 3, H, W), dtype=torch.float32, device=device)
                side = torch.cuda.Stream(device)            # warm-up off the capture stream (allocator, lazy init, packing)
                side.wait_stream(stream)
                with torch.cuda.stream(side):
                    model(self.left, self.right)
                stream.wait_stream(side)
                self.graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(self.graph):
                    self.pred = model(self.left, self.right)[-1]
        finally:
            model.max_disp = saved
        self.held = _cache_tensors(model)
        if tuple(self.pred.shape) != (B, H, W) or not self.pred.is_contiguous():
            raise RuntimeError("the model returned a disparity map of shape %s, expected %s"
                               % (tuple(self.pred.shape), (B, H, W)))


def _cache_tensors(model):
    """Every tensor the caches of ``model``'s modules hold (stage0.CachesWeights.cache_tensors: packed weights, workspaces)."""
    from .stage0 import CachesWeights
    return [t for m in model.modules() if isinstance(m, CachesWeights) for t in m.cache_tensors()]


def fill_batch(dst, items, repeat_last=True):
    """dst[i] = items[i]; the rows past len(items) take the last item (a short batch runs as a full one whose extra outputs
    are dropped) or, without ``repeat_last``, zeros."""
    n = len(items)
    for i in range(len(dst)):
        dst[i] = items[min(i, n - 1)] if (i < n or repeat_last) else 0


class _Slot:
    """The staging of one batch in flight.  Buffers are flat and grow to the largest batch the slot has carried."""

    def __init__(self):
        self.busy = False
        self.tag = self.shape = self.n = None
        self.has_gt = False
        self.sums_out = None
        self.buf = {}

    def flat(self, name, n, dtype, device=None):
        t = self.buf.get(name)
        if t is None or t.numel() < n:
            t = torch.empty(n, dtype=dtype, device=device) if device is not None else \
                torch.empty(n, dtype=dtype, pin_memory=True)
            self.buf[name] = t
        return t[:n]


class _HipBackend:
    """Everything of the engine that touches the device."""

    def __init__(self, model):
        p = next(model.parameters(), None)
        if p is None or not p.is_cuda:
            raise ValueError("StereoEngine needs a model on the MI355X (there is no CPU path)")
        self.model, self.device = model, p.device
        with torch.cuda.device(self.device):
            self.compute = torch.cuda.Stream(self.device)
            self.copy = torch.cuda.Stream(self.device)
            self.compute.wait_stream(torch.cuda.current_stream(self.device))     # weights uploaded on the caller's stream
        self.table = imageio.normalise_table().to(self.device)
        torch.cuda.current_stream(self.device).synchronize()

    def new_slot(self):
        s = _Slot()
        s.ev_up, s.ev_comp, s.ev_done = (torch.cuda.Event() for _ in range(3))
        return s

    def new_bucket(self, key):
        self.compute.synchronize()          # the warm-up runs eagerly through workspaces that graphs in flight may use
        self.compute.wait_stream(torch.cuda.current_stream(self.device))         # weight writes on the caller's stream
        with torch.cuda.device(self.device):
            return _Bucket(self.model, key, self.device, self.compute)

    def drop_bucket(self, bucket):
        if bucket.last_use is not None:
            bucket.last_use.synchronize()   # a graph is not destroyed under its own replay

    def stage(self, slot, lefts, rights, gts, B, sums_out=None):
        """Host work only: the views (and ground truth) into the slot's pinned staging; the batch filled up to B."""
        n = len(lefts)
        h, w = lefts[0].shape[:2]
        u8 = slot.flat("u8_host", 2 * B * h * w * 3, torch.uint8).numpy().reshape(2, B, h, w, 3)
        fill_batch(u8[0], lefts)
        fill_batch(u8[1], rights)
        if gts is not None:                                                   # a filled sample has no valid pixel
            fill_batch(slot.flat("gt_host", B * h * w, torch.float32).numpy().reshape(B, h, w), gts, repeat_last=False)
        slot.shape, slot.n, slot.has_gt, slot.sums_out = (B, h, w), n, gts is not None, sums_out

    def upload(self, slot):
        B, h, w = slot.shape
        dev = self.device
        with torch.cuda.device(dev), torch.cuda.stream(self.copy):
            slot.flat("u8_dev", 2 * B * h * w * 3, torch.uint8, dev).copy_(
                slot.flat("u8_host", 2 * B * h * w * 3, torch.uint8), non_blocking=True)
            if slot.has_gt:
                slot.flat("gt_dev", B * h * w, torch.float32, dev).copy_(
                    slot.flat("gt_host", B * h * w, torch.float32), non_blocking=True)
            slot.ev_up.record(self.copy)

    def compute_batch(self, slot, bucket):
        B, h, w = slot.shape
        dev = self.device
        if slot.sums_out is not None:                       # the caller's tensor: behind what the caller's stream did to it
            self.compute.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.device(dev), torch.cuda.stream(self.compute), torch.no_grad():
            self.compute.wait_event(slot.ev_up)
            u8 = slot.flat("u8_dev", 2 * B * h * w * 3, torch.uint8, dev).view(2, B, h, w, 3)
            imageio.preprocess_u8(u8[0], self.table, bucket.left)
            imageio.preprocess_u8(u8[1], self.table, bucket.right)
            bucket.graph.replay()
            imageio.disparity_to_u16(bucket.pred, slot.flat("u16_dev", B * h * w, torch.int16, dev).view(B, h, w))
            if slot.has_gt:
                part = slot.flat("part_dev", B * h * 3, torch.float32, dev).view(B, h, 3)
                imageio.disparity_metrics(bucket.pred, slot.flat("gt_dev", B * h * w, torch.float32, dev).view(B, h, w),
                                          bucket.key[3], part)
                sums = slot.sums_out if slot.sums_out is not None else slot.flat("sums_dev", 3, torch.float64, dev)
                sums.copy_(imageio.sums_from_partials(part))
            slot.ev_comp.record(self.compute)
        bucket.last_use = slot.ev_comp

    def download(self, slot):
        B, h, w = slot.shape
        dev = self.device
        with torch.cuda.device(dev), torch.cuda.stream(self.copy):
            self.copy.wait_event(slot.ev_comp)
            slot.flat("u16_host", B * h * w, torch.int16).copy_(slot.flat("u16_dev", B * h * w, torch.int16, dev),
                                                                 non_blocking=True)
            if slot.has_gt and slot.sums_out is None:
                slot.flat("sums_host", 3, torch.float64).copy_(slot.flat("sums_dev", 3, torch.float64, dev),
                                                               non_blocking=True)
            slot.ev_done.record(self.copy)

    def computed(self, slot):
        return slot.ev_comp.query()

    def done(self, slot):
        return slot.ev_done.query()

    def wait(self, slot):
        slot.ev_done.synchronize()

    def collect(self, slot):
        """Host work only: the finished batch out of the pinned staging (copies: the slot is reused)."""
        B, h, w = slot.shape
        out = np.array(slot.flat("u16_host", B * h * w, torch.int16).numpy().view(np.uint16).reshape(B, h, w)[:slot.n])
        metrics = None
        if slot.has_gt and slot.sums_out is None:
            metrics = imageio.metrics_from_sums(slot.flat("sums_host", 3, torch.float64).numpy())
        slot.sums_out = None
        return list(out), metrics


class StereoEngine:
    """See the module docstring.  ``model``: a ``use_detail`` network on the GPU, in eval mode."""

    def __init__(self, model, batch_size=8, depth=2, max_buckets=4, backend=None):
        if not getattr(model, "use_detail", False):
            raise ValueError("StereoEngine runs use_detail models only: host detail masks are a different input contract")
        if batch_size < 1 or depth < 1 or max_buckets < 1:
            raise ValueError("batch_size, depth and max_buckets must be >= 1")
        self.model, self.batch_size, self.depth, self.max_buckets = model, int(batch_size), int(depth), int(max_buckets)
        self._dev = _HipBackend(model) if backend is None else backend
        self._buckets = collections.OrderedDict()           # key -> bucket, least recently used first
        self._slots = [self._dev.new_slot() for _ in range(self.depth)]
        self._order = collections.deque()                   # busy slots, oldest submission first
        self._undownloaded = None                           # the slot whose D2H is not on the copy stream yet
        self._finished = collections.deque()
        self._count = 0

    # ---- buckets -------------------------------------------------------------------------------------------------------
    def bucket_key(self, h, w, max_disp=None):
        H, W = imageio.padded_size(h, w)
        return (self.batch_size, H, W, int(self.model.max_disp if max_disp is None else max_disp))

    def _bucket(self, key):
        b = self._buckets.get(key)
        if b is None:
            while len(self._buckets) >= self.max_buckets:
                self._dev.drop_bucket(self._buckets.popitem(last=False)[1])
            b = self._buckets[key] = self._dev.new_bucket(key)
        else:
            self._buckets.move_to_end(key)
        return b

    def reset(self):
        """Drop every bucket (waits for what is in flight; finished results stay available to results() / flush())."""
        self._retire(wait=True)
        while self._buckets:
            self._dev.drop_bucket(self._buckets.popitem(last=False)[1])

    # ---- batches -------------------------------------------------------------------------------------------------------
    def submit(self, lefts, rights, max_disp=None, gts=None, tag=None, sums_out=None):
        """Queue one batch: lists of equal-size h x w x 3 uint8 arrays, at most batch_size of them.  max_disp: the
        disparity range (None: model.max_disp as it is now).  gts: h x w float32 ground truth per pair; the result then
        carries (epe, loss_3) over the batch.  sums_out: a float64 [3] tensor on the model's device that receives the
        batch's (valid count, sum of errors, good count) INSTEAD -- nothing of the metrics is read back, and the tensor is
        complete once the batch has come back from results() / flush() (eval keeps one [n_batches, 3] record this way).
        The write is ordered behind the work queued so far on the stream that is current in this call."""
        lefts, rights = list(lefts), list(rights)
        if gts is not None:
            gts = list(gts)
        if sums_out is not None and (gts is None or not isinstance(sums_out, torch.Tensor) or
                                     sums_out.dtype != torch.float64 or tuple(sums_out.shape) != (3,)):
            raise ValueError("sums_out must be a float64 [3] tensor and needs gts")
        n = len(lefts)
        if not 1 <= n <= self.batch_size or len(rights) != n or (gts is not None and len(gts) != n):
            raise ValueError("a batch is 1 .. %d pairs (got %d left, %d right views)" % (self.batch_size, n, len(rights)))
        shape = lefts[0].shape
        if len(shape) != 3 or shape[2] != 3:
            raise ValueError("views must be h x w x 3 arrays, got %s" % (shape,))
        for a in lefts + rights:
            if a.shape != shape or a.dtype != np.uint8:
                raise ValueError("the views of a batch must be uint8 arrays of one size")
        if gts is not None and any(g.shape != shape[:2] for g in gts):
            raise ValueError("ground truth must be h x w, the size of the views")
        slot = self._slots[self._count % self.depth]
        if slot.busy:                                       # every slot in flight: wait for the oldest
            self._retire(wait=True, upto=slot)
        bucket = self._bucket(self.bucket_key(shape[0], shape[1], max_disp))
        self._dev.stage(slot, lefts, rights, gts, self.batch_size, sums_out)
        slot.busy, slot.tag = True, tag
        self._dev.upload(slot)
        self._download_pending()                            # behind this batch's upload on the copy stream
        self._dev.compute_batch(slot, bucket)
        self._undownloaded = slot
        self._order.append(slot)
        self._count += 1

    def _download_pending(self):
        if self._undownloaded is not None:
            self._dev.download(self._undownloaded)
            self._undownloaded = None

    def _retire(self, wait, upto=None):
        """Move finished batches, oldest first, to the result queue; with ``wait`` up to and including ``upto`` (None: all)."""
        while self._order:
            slot = self._order[0]
            if slot is self._undownloaded:
                if not wait and not self._dev.computed(slot):
                    break                                   # its D2H would hold the copy stream until it has computed
                self._download_pending()
            if wait:
                self._dev.wait(slot)
            elif not self._dev.done(slot):
                break
            self._order.popleft()
            arrays, metrics = self._dev.collect(slot)
            self._finished.append((slot.tag, arrays, metrics))
            slot.busy, slot.tag = False, None
            if slot is upto:
                break

    def results(self):
        """The batches finished so far, in submission order: [(tag, [h x w uint16 arrays], metrics or None)].  Never
        blocks.  ``metrics`` is (epe, loss_3) of eval.test_loss_func over the batch where ground truth was submitted."""
        self._retire(wait=False)
        out = list(self._finished)
        self._finished.clear()
        return out

    def flush(self):
        """Wait for every submitted batch and return the results not handed out yet."""
        self._retire(wait=True)
        out = list(self._finished)
        self._finished.clear()
        return out
