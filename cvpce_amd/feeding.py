"""Input pipeline of the product path: shelf images are read ahead by worker threads and, in the 8-bit form, uploaded from pinned
memory on a copy stream while the kernels work on the images before them.

    for image, planogram in ImageFeeder(pairs, workers=8, device='cuda'):
        ...                                  # image: uint8 (H,W,3) on the device; the kernels read it there (ops.input_image)

The counterpart of the reference's `DataLoader(num_workers=..., pin_memory=True)` for the evaluation loops, in one process: PIL
releases the GIL while it decodes, so threads are enough (`Classifier._gallery_items` is the same pattern for the gallery).  One GPU
context, one extra stream, no processes.
"""
from collections import deque
from concurrent.futures import ThreadPoolExecutor

import torch

from . import ops

DEFAULT_WORKERS = 8     # the reference's DataLoader default
MAX_WORKERS = 16        # never sized by os.cpu_count(): a job is given far fewer CPUs than the machine shows
DEFAULT_DEPTH = 4       # images uploaded ahead of the consumer = slots of the pinned ring


def _image_of(item):
    return item[0] if isinstance(item, (tuple, list)) else item


def _with_image(item, image):
    if isinstance(item, tuple):
        return (image,) + item[1:]
    if isinstance(item, list):
        return [image] + item[1:]
    return image


def feed(dataset, num_workers, device='cuda'):
    """`dataset` read through an ImageFeeder with `num_workers` threads; as it is when num_workers is 0 / None (the serial in-process
    reading) or it is a feeder already.  What the evaluation functions do with their `num_workers` argument."""
    if not num_workers or num_workers <= 0 or isinstance(dataset, ImageFeeder):
        return dataset
    return ImageFeeder(dataset, workers=num_workers, device=device)


class _Serial:
    """A read made in the calling thread when its result is asked for (workers = 0, or a source that cannot be indexed)."""

    def __init__(self, fn):
        self.result = fn

    @staticmethod
    def done():
        return False


class _Slot:
    """One pinned staging buffer of the ring + the event after which the host may refill it (its upload has been read)."""

    def __init__(self):
        self.buffer = None
        self.uploaded = None

    def stage(self, image):
        """-> a pinned view holding `image`'s bytes; the buffer is reused while the size fits and reallocated when an image is larger."""
        if self.uploaded is not None:
            self.uploaded.synchronize()          # (the only host wait of the feeder: for a slot whose last upload is still travelling)
        n = image.numel()
        if self.buffer is None or self.buffer.numel() < n:
            self.buffer = torch.empty(n, dtype=torch.uint8).pin_memory()
        view = self.buffer[:n].view(image.shape)
        view.copy_(image)
        return view


class ImageFeeder:
    """Iterates `source` -- an indexable dataset (`len` + `[i]`) or any iterable of items -- in order and yields each item with its
    image (the item itself, or its first element) replaced by a device-resident one.

    workers: threads that call `source[i]` a bounded window ahead (at most `depth + workers` items are read and not yet yielded);
        0 reads in the calling thread.  Default 8, capped at 16.  An iterable that cannot be indexed is read in the calling thread.
    depth:   8-bit images uploaded ahead of the consumer (default 4).  They go through a ring of `depth + workers` pinned buffers (one
        per read that can be outstanding; the reader that decoded an image also copies it into its slot) and ONE copy stream owned
        by the feeder, one event per slot; the consumer's stream waits on that event when the item is yielded, so what the caller
        launches next reads the finished upload without a host synchronisation.
    device:  None or a CPU device: no pinning, no upload, host images are yielded (the threading alone).

    Float images pass through as they are (the entry points upload them as before): the feeder is about reading ahead.
    Order is the source's whatever the per-item latency; an exception raised by `source[i]` is raised at position i, after the items
    before it.  Leaving the loop early (`break`, `close()`) stops and joins the workers and frees the ring."""

    def __init__(self, source, workers=DEFAULT_WORKERS, depth=None, device=None):
        self.source = source
        self.workers = max(0, min(int(workers), MAX_WORKERS))
        self.depth = max(1, int(depth)) if depth is not None else DEFAULT_DEPTH
        device = torch.device(device) if device is not None else None
        self.device = device if device is not None and device.type != 'cpu' else None
        self.indexable = hasattr(source, '__getitem__') and hasattr(source, '__len__')
        self.bytes_uploaded = 0          # 8-bit image bytes sent to the device so far (tools/bench_input_path.py reads it)

    def __len__(self):
        return len(self.source)

    # -- reading ------------------------------------------------------------------------------------------------------
    def _read(self, get, slot):
        """One read, in whichever thread runs it: the item, and -- with a ring slot and a host 8-bit image -- its bytes staged in the
        slot's pinned buffer, so that the copy into pinned memory is the readers' work too, not the consumer's.
        -> (item, pinned view | None, slot, exception | None); never raises (the exception is raised at the item's position)."""
        try:
            item = get()
            image = _image_of(item)
            staged = None
            if slot is not None and ops.is_uint8_image(image) and not image.is_cuda:
                staged = slot.stage(ops.check_image_form(image))
            return item, staged, slot, None
        except Exception as e:
            return None, None, slot, e

    def _read_ahead(self, free):
        """-> generator of reads, one per item in order: `.result()` returns what `_read` returns, `.done()` tells whether that would
        not block.  With workers, at most `depth + workers` reads are started and not yet yielded to the consumer, counting those
        the upload stage holds; every such read owns one slot of `free` (the ring has that many), None without a device."""
        take = (lambda: free.pop()) if free is not None else (lambda: None)
        if not self.indexable:
            for item in self.source:
                yield _Serial(lambda item=item: self._read(lambda: item, take()))
            return
        n = len(self.source)
        if self.workers <= 0:
            for i in range(n):
                yield _Serial(lambda i=i: self._read(lambda: self.source[i], take()))
            return
        pool = ThreadPoolExecutor(self.workers, thread_name_prefix='cvpce-feeder')
        pending, nxt = deque(), 0
        try:
            while nxt < n or pending:
                while nxt < n and len(pending) + self._held < self.depth + self.workers:
                    pending.append(pool.submit(self._read, (lambda i=nxt: self.source[i]), take()))
                    nxt += 1
                yield pending.popleft()
        finally:
            for f in pending:
                f.cancel()
            pool.shutdown(wait=True, cancel_futures=True)

    # -- uploading ----------------------------------------------------------------------------------------------------
    def _upload(self, staged, slot, stream):
        """pinned 8-bit image -> (device tensor, event recorded behind its upload on the copy stream)."""
        with torch.cuda.stream(stream):
            on_device = torch.empty(staged.shape, dtype=torch.uint8, device=self.device)
            on_device.copy_(staged, non_blocking=True)
            done = torch.cuda.Event()
            done.record(stream)
        slot.uploaded = done
        self.bytes_uploaded += staged.numel()
        return on_device, done

    def __iter__(self):
        self._held = 0                     # items read and handed to the upload stage, not yet yielded
        if self.device is None:
            reads = self._read_ahead(None)
            try:
                for read in reads:
                    item, _, _, error = read.result()
                    if error is not None:
                        raise error
                    yield item
            finally:
                reads.close()
            return
        # the ring: one slot per read that can be outstanding, so a read never waits for a slot -- only, inside `stage`, for the
        # upload that last used its slot (an event that completes on its own: nothing here can wait on the consumer)
        free = [_Slot() for _ in range(self.depth + max(self.workers, 1))]
        reads = self._read_ahead(free)
        stream = torch.cuda.Stream(device=self.device)
        held = deque()                     # (item, device image | None, event | None, slot, exception | None), uploads issued
        head, exhausted = None, False      # the next read, taken from `reads` and not yet in `held`
        try:
            while True:
                # top up: every read that has finished is uploaded before the consumer gets its item, so that image i + 1 travels
                # while image i is computed; the host only waits for a read when it has nothing to hand over
                while not exhausted and len(held) < self.depth and not (held and held[-1][4] is not None):
                    if head is None:
                        try:
                            head = next(reads)
                        except StopIteration:
                            exhausted = True
                            break
                    if held and not head.done():
                        break
                    (item, staged, slot, error), head = head.result(), None
                    on_device, done = self._upload(staged, slot, stream) if staged is not None else (None, None)
                    held.append((item, on_device, done, slot, error))
                    self._held = len(held)
                self._held = len(held) + (head is not None)
                if not held:
                    return
                item, on_device, done, slot, error = held.popleft()
                free.append(slot)          # (its pinned bytes may still be travelling: the next `stage` of this slot waits for `done`)
                self._held = len(held) + (head is not None)
                if error is not None:
                    raise error
                if on_device is not None:
                    consumer = torch.cuda.current_stream(self.device)
                    consumer.wait_event(done)
                    # allocated on the copy stream, read on the consumer's: not recycled in flight.  With ops.U8_KERNELS on the bytes are
                    # read not by one conversion but by the transform and, later, by every crop launch -- all on this stream (the
                    # detector's side streams read feature maps, never the image), and the allocator holds the block until the work
                    # queued on this stream WHEN THE TENSOR IS FREED has run: one record covers them all
                    on_device.record_stream(consumer)
                    item = _with_image(item, on_device)
                yield item
        finally:
            reads.close()
            held.clear()
            free.clear()
