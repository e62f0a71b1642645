"""The input path of training from scratch: planned batches -> staged record bytes -> packed float32 batches on the device.

head_train.read_train_batch decodes every utterance of a batch whole, in Python, to keep `length` rows of it.  Here the host
only copies bytes: xv_train_stage (csrc/train_stage.cpp) preads what the chunks of a batch need out of the archives into a
pinned buffer -- for Kaldi's compressed records one byte per element -- and xv_train_batch_decode (csrc/train_batch.hip) turns
them into the [B * length, dim] batch in one launch, with the bits the native reader (csrc/ark_io.cpp) decodes.  What the
reference does with worker processes and dataset/kaldi_io.py:1118-1171 (_read_compressed_submat).

A chunk the stager refuses (a piped or ranged rxfilename, a record it cannot read) is read with kaldi_io.read_mat as
read_train_batch would and staged as a float payload, so every input head_train.train_head accepts still works.

`Loader` iterates over head_train.plan_train_batches (the deterministic stand-in for KaldiDataRandomQueue, **parity unpinned**):
a batch is a pure function of the plan, the same bits for every `prefetch`, thread count and repeat."""
import ctypes as C
import queue
import threading

import numpy as np

from . import _lib

STAGE_THREADS = 16


def _align16(n):
    return (int(n) + 15) & ~15


class StagedBatch(object):
    """Descriptors (a ctypes array of _lib.TrainChunk), the staged byte count, and which chunks went through read_mat."""

    def __init__(self, chunks, nbytes, fallbacks):
        self.chunks, self.nbytes, self.fallbacks = chunks, int(nbytes), fallbacks


def stage(rxfiles, starts, length, buf, threads=STAGE_THREADS):
    """xv_train_stage on `buf` (a writable uint8 numpy array) -> (return code, chunks, status int32 [n], staged bytes, message).
    Nothing is raised: the caller decides what a refused chunk means."""
    lib = _lib.load()
    n = len(rxfiles)
    if any("\n" in rx for rx in rxfiles):
        raise ValueError("an rxfilename holds a newline")
    chunks = (_lib.TrainChunk * n)()
    status = np.zeros(n, dtype=np.int32)
    starts = np.ascontiguousarray(starts, dtype=np.int32)
    nbytes = C.c_int64(0)
    err = C.create_string_buffer(1024)
    rc = lib.xv_train_stage(("\n".join(rxfiles) + "\n").encode(), n, starts.ctypes.data_as(C.c_void_p), int(length), int(threads),
                            buf.ctypes.data_as(C.c_void_p), buf.size, C.cast(chunks, C.c_void_p), status.ctypes.data_as(C.c_void_p),
                            C.cast(C.pointer(nbytes), C.c_void_p), C.cast(err, C.c_void_p), len(err))
    return int(rc), chunks, status, int(nbytes.value), err.value.decode("utf-8", "replace")


def stage_batch(batch, dim, reserve, threads=STAGE_THREADS):
    """Stage one head_train.TrainBatch.  reserve(nbytes) -> a writable uint8 numpy array of at least nbytes (it may hand back
    the same array while it is large enough; what it held need not survive a growth).  -> (array, StagedBatch)."""
    from .kaldi_io import read_mat
    n = len(batch.keys)
    buf = reserve(1 << 16)
    rc, chunks, status, nbytes, msg = stage(batch.rxfiles, batch.starts, batch.length, buf, threads)
    if rc == _lib.XV_ERR_WORKSPACE:
        buf = reserve(nbytes)
        rc, chunks, status, nbytes, msg = stage(batch.rxfiles, batch.starts, batch.length, buf, threads)
    if rc < 0:
        raise IOError("staging the batch failed: %s" % msg)
    fallbacks = []
    if rc > 0:                                                   # refused chunks: read them as read_train_batch does
        mats, total = [], nbytes
        for j in np.nonzero(status)[0]:
            key, rx, start = batch.keys[j], batch.rxfiles[j], int(batch.starts[j])
            mat = read_mat(rx)
            if mat.shape[0] < start + batch.length:
                raise ValueError("%s: %d frames in the archive, utt2num_frames promised at least %d" % (key, mat.shape[0], start + batch.length))
            mats.append((int(j), total, np.ascontiguousarray(mat[start:start + batch.length], dtype=np.float32)))
            total = _align16(total + mats[-1][2].nbytes)
        if total > buf.size:                                     # grow, then stage the native chunks again behind the same layout
            buf = reserve(total)
            rc, chunks, status, nbytes, msg = stage(batch.rxfiles, batch.starts, batch.length, buf, threads)
            if rc < 0:
                raise IOError("staging the batch failed: %s" % msg)
        for j, off, rows in mats:
            buf[off:off + rows.nbytes] = rows.reshape(-1).view(np.uint8)
            c = chunks[j]
            c.kind, c.cols, c.rows, c.first_row, c.payload_off, c.header_off = _lib.XV_TRAIN_FM, rows.shape[1], rows.shape[0], 0, off, 0
            fallbacks.append(j)
        nbytes = total
    for j in range(n):
        if chunks[j].cols < dim:
            raise ValueError("%s: features have %d columns, the network needs %d" % (batch.keys[j], chunks[j].cols, dim))
    return buf, StagedBatch(chunks, nbytes, fallbacks)


def decode(staged_dev, nbytes, chunks, length, dim, out, ws, device, ld=None):
    """xv_train_batch_decode on torch's current stream of `device`: staged_dev (uint8 device tensor), chunks (ctypes array of
    _lib.TrainChunk) -> rows [n * length, :dim] of `out` (float32 device tensor of leading dimension ld, default its row stride)."""
    lib = _lib.load()
    ld = int(out.stride(0)) if ld is None else int(ld)
    _lib.check(lib.xv_train_batch_decode(int(device), _lib.ptr(staged_dev), int(nbytes), C.cast(chunks, C.c_void_p), len(chunks),
                                         int(length), int(dim), _lib.ptr(out), ld, _lib.ptr(ws), ws.numel(), _lib.stream(device)))
    return out


def workspace_bytes(num_chunks):
    return int(_lib.load().xv_train_batch_workspace(int(num_chunks)))


class _Slot(object):
    """One turn of the ring: a pinned staging buffer, its device copy, the decoded batch and the two events."""

    def __init__(self, torch, device):
        self.torch, self.device = torch, device
        self.pinned = self.array = self.staged_dev = self.out = self.ws = None
        self.ready = torch.cuda.Event()              # the upload and the decode of this turn are done
        self.released = None                         # the consumer's stream is done with `out`

    def reserve(self, nbytes):
        if self.array is None or self.array.size < nbytes:
            size = max(1 << 20, 1 << (int(nbytes) - 1).bit_length())
            self.pinned = self.torch.empty(size, dtype=self.torch.uint8).pin_memory()
            self.array = self.pinned.numpy()
            self.staged_dev = self.torch.empty(size, dtype=self.torch.uint8, device=self.device)
        return self.array


class Loader(object):
    """for feats_dev, offsets, labels, batch in Loader(...).epoch(e): the batches of head_train.plan_train_batches(train_dir,
    spklist, params, seed, e), each decoded on the device into float32 [B * length, dim]; offsets = arange(B + 1) * length.
    With prefetch > 0 one worker thread stages, uploads and decodes up to `prefetch` batches ahead on a side stream while the
    consumer's step runs; the consumer's stream waits on the batch's event.  prefetch = 0 does the same work inline.  A yielded
    batch stays valid until the next one is asked for.  No processes, at most one thread."""

    def __init__(self, train_dir, spklist, params, seed, dim, device=0, prefetch=2, threads=STAGE_THREADS):
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("train_input.Loader needs a HIP device: the batch former has no CPU path")
        if prefetch < 0:
            raise ValueError("prefetch must not be negative, got %r" % (prefetch,))
        self.train_dir, self.spklist, self.params, self.seed = train_dir, spklist, params, seed
        self.dim, self.device, self.prefetch, self.threads = int(dim), int(device), int(prefetch), int(threads)
        self._torch = torch
        self._dev = torch.device("cuda:%d" % self.device)
        with torch.cuda.device(self.device):
            self._side = torch.cuda.Stream(self.device)
            self._slots = [_Slot(torch, self._dev) for _ in range(self.prefetch + 1)]

    def _make(self, slot, batch):
        """Stage, upload, decode `batch` into `slot` on the side stream; the slot's ready event closes it."""
        torch = self._torch
        n = len(batch.keys)
        slot.ready.synchronize()                                     # the previous upload out of this pinned buffer
        _, staged = stage_batch(batch, self.dim, slot.reserve, self.threads)
        with torch.cuda.device(self.device):
            rows = n * batch.length
            if slot.out is None or slot.out.shape[0] < rows:
                slot.out = torch.empty((rows, self.dim), dtype=torch.float32, device=self._dev)
            need = workspace_bytes(n)
            if slot.ws is None or slot.ws.numel() < need:
                slot.ws = torch.empty(need, dtype=torch.uint8, device=self._dev)
            with torch.cuda.stream(self._side):
                if slot.released is not None:
                    self._side.wait_event(slot.released)
                slot.staged_dev[:staged.nbytes].copy_(slot.pinned[:staged.nbytes], non_blocking=True)
                decode(slot.staged_dev, staged.nbytes, staged.chunks, batch.length, self.dim, slot.out, slot.ws, self.device)
                slot.ready.record(self._side)
        return slot.out[:rows]

    def _deliver(self, slot, feats, batch):
        torch = self._torch
        with torch.cuda.device(self.device):
            torch.cuda.current_stream(self.device).wait_event(slot.ready)
        offsets = np.arange(len(batch.keys) + 1, dtype=np.int64) * batch.length
        return feats, offsets, batch.labels, batch

    def _release(self, slot):
        torch = self._torch
        with torch.cuda.device(self.device):
            slot.released = torch.cuda.Event()
            slot.released.record(torch.cuda.current_stream(self.device))

    def epoch(self, epoch, skip=0):
        """The batches of `epoch`, the first `skip` of its plan left out (a run that continues inside an epoch)."""
        from .head_train import plan_train_batches
        plan = plan_train_batches(self.train_dir, self.spklist, self.params, self.seed, epoch)[int(skip):]
        return self.batches(plan)

    def batches(self, plan):
        if self.prefetch == 0:
            slot = self._slots[0]
            for batch in plan:
                feats = self._make(slot, batch)
                yield self._deliver(slot, feats, batch)
                self._release(slot)
            return
        free, ready, stop = queue.Queue(), queue.Queue(), threading.Event()
        for s in self._slots:
            free.put(s)

        def work():
            try:
                for batch in plan:
                    slot = free.get()
                    if slot is None or stop.is_set():
                        return
                    ready.put((slot, self._make(slot, batch), batch))
                ready.put(None)
            except BaseException as e:                               # handed to the consumer, which raises it
                ready.put(e)

        worker = threading.Thread(target=work, name="train-input", daemon=True)
        worker.start()
        held = None
        try:
            while True:
                item = ready.get()
                if item is None:
                    break
                if isinstance(item, BaseException):
                    raise item
                slot, feats, batch = item
                held = slot
                yield self._deliver(slot, feats, batch)
                self._release(slot)
                held = None
                free.put(slot)
        finally:
            stop.set()
            free.put(None)
            if held is not None:
                self._release(held)
            worker.join()
            self._torch.cuda.synchronize(self.device)
