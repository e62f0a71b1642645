#!/usr/bin/env python
"""Time the input path of training beside the step it feeds.  The numbers of profiles/train.md come from this tool:

    python tools/train_input_bench.py [--utts 2000] [--speakers 200] [--segments 64] [--frames 300] [--dim 30] [--batches 10]
                                      [--steps 30] [--rounds 3] [--dir D]

It writes a synthetic set of 'CM ' archives (Kaldi's compressed matrices, the format training features are kept in: random
headers and bytes, every byte string is a valid record) of --utts utterances of 400 to 1 000 frames on local disk, plans batches
of --segments chunks of --frames frames with head_train.plan_train_batches, and times, as medians of --rounds alternating rounds:

  parent   head_train.read_train_batch (kaldi_io.read_mat per chunk) and the upload of head_train._conv_step, per batch;
  new      train_input's stage, upload and decode (xv_train_stage, one copy, xv_train_batch_decode), per batch; its staging alone;
  kernel   xv_train_batch_decode alone on a resident staged batch (device events around back-to-back launches), beside a device
           copy that moves as many bytes as the kernel reads and writes;
  steps    ConvTrainer.step fed by train_input.Loader with prefetch 0 and 2, and by the parent's path, beside the bare step on a
           resident batch: steps per second.

Host-side figures are a host clock around work that ends in a device synchronise.  Nothing is gated; one JSON line at the end."""
import argparse
import json
import os
import struct
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def write_set(root, utts, speakers, dim, rs, per_ark=250):
    """feats.scp, spk2utt, utt2num_frames and a spklist over 'CM ' archives of random bytes -> (data dir, spklist path)."""
    data = os.path.join(root, "data")
    os.makedirs(data, exist_ok=True)
    scp, frames, spk2utt = [], [], [[] for _ in range(speakers)]
    f = None
    for i in range(utts):
        if i % per_ark == 0:
            if f is not None:
                f.close()
            ark = os.path.join(data, "feats.%d.ark" % (i // per_ark))
            f = open(ark, "wb")
        key = "spk%04d-utt%05d" % (i % speakers, i)
        rows = int(rs.randint(400, 1001))
        f.write(key.encode() + b" ")
        scp.append("%s %s:%d\n" % (key, ark, f.tell()))
        f.write(b"\0BCM " + struct.pack("<ffii", -20.0, 40.0, rows, dim))
        f.write(np.sort(rs.randint(0, 65536, (dim, 4)), axis=1).astype(np.uint16).tobytes())
        f.write(rs.randint(0, 256, (dim, rows)).astype(np.uint8).tobytes())
        frames.append((key, rows))
        spk2utt[i % speakers].append(key)
    f.close()
    with open(os.path.join(data, "feats.scp"), "w") as g:
        g.writelines(scp)
    with open(os.path.join(data, "utt2num_frames"), "w") as g:
        g.writelines("%s %d\n" % kv for kv in frames)
    with open(os.path.join(data, "spk2utt"), "w") as g:
        g.writelines("spk%04d %s\n" % (s, " ".join(u)) for s, u in enumerate(spk2utt))
    spklist = os.path.join(root, "spklist")
    with open(spklist, "w") as g:
        g.writelines("spk%04d %d\n" % (s, s) for s in range(speakers))
    return data, spklist


def median_rounds(rounds):
    return {k: float(np.median([r[k] for r in rounds])) for k in rounds[0]}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=2000)
    ap.add_argument("--speakers", type=int, default=200)
    ap.add_argument("--segments", type=int, default=64)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--dim", type=int, default=30)
    ap.add_argument("--batches", type=int, default=10)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--kernel-iters", type=int, default=200)
    ap.add_argument("--channels", type=int, default=512)
    ap.add_argument("--dir", type=str, default="")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args(argv)
    import torch
    from tf_kaldi_speaker_amd import head_train, synth, train, train_input
    from tf_kaldi_speaker_amd.params import Params
    if not torch.cuda.is_available():
        sys.exit("train_input_bench.py needs a HIP device: nothing here is timed on a CPU")
    torch.backends.cuda.matmul.allow_tf32 = False
    dev = "cuda:%d" % args.device
    root = args.dir or tempfile.mkdtemp(prefix="train_input_bench.")
    rs = np.random.RandomState(0)
    data, spklist = write_set(root, args.utts, args.speakers, args.dim, rs)
    p = dict(synth.TDNN_STAT_PARAMS, num_speakers_per_batch=args.segments, num_segments_per_speaker=1, min_segment_len=args.frames,
             max_segment_len=args.frames, num_steps_per_epoch=max(args.batches, args.steps), optimizer="momentum", momentum=0.9,
             learning_rate=0.01, weight_l2_regularizer=1e-4)
    params = Params(**p)
    plan = head_train.plan_train_batches(data, spklist, params, 0, 0)
    n, length, dim = args.segments, args.frames, args.dim
    sync = lambda: torch.cuda.synchronize(args.device)                                   # noqa: E731

    def parent_batch(batch):
        feats = head_train.read_train_batch(batch, dim)
        return torch.from_numpy(np.ascontiguousarray(feats, dtype=np.float32).reshape(n * length, dim)).to(dev)

    loader = train_input.Loader(data, spklist, params, 0, dim, args.device, prefetch=0)
    slot = loader._slots[0]
    # ---- per batch: the parent's path, the new path, the staging alone
    for batch in plan[:2]:                                                                # warm-up: page cache, allocations, code objects
        parent_batch(batch)
        loader._make(slot, batch)
    sync()
    rounds = []
    for _ in range(args.rounds):
        r = {}
        t0 = time.perf_counter()
        for batch in plan[:args.batches]:
            parent_batch(batch)
        sync()
        r["parent_ms"] = (time.perf_counter() - t0) * 1e3 / args.batches
        t0 = time.perf_counter()
        for batch in plan[:args.batches]:
            loader._make(slot, batch)
        sync()
        r["new_ms"] = (time.perf_counter() - t0) * 1e3 / args.batches
        t0 = time.perf_counter()
        for batch in plan[:args.batches]:
            _, staged = train_input.stage_batch(batch, dim, slot.reserve)
        r["stage_ms"] = (time.perf_counter() - t0) * 1e3 / args.batches
        rounds.append(r)
    per_batch = median_rounds(rounds)
    # the two paths give the same batch (kaldi_io's numpy decode and the native rule agree bit for bit)
    same = bool(np.array_equal(parent_batch(plan[0]).cpu().numpy().view(np.uint32), loader._make(slot, plan[0]).cpu().numpy().view(np.uint32)))
    # ---- the kernel alone, beside a device copy of the bytes it moves
    _, staged = train_input.stage_batch(plan[0], dim, slot.reserve)
    slot.staged_dev[:staged.nbytes].copy_(slot.pinned[:staged.nbytes])
    out = torch.empty((n * length, dim), dtype=torch.float32, device=dev)
    ws = torch.empty(train_input.workspace_bytes(n), dtype=torch.uint8, device=dev)
    in_bytes, out_bytes = n * length * dim + n * dim * 8, n * length * dim * 4
    half = (in_bytes + out_bytes) // 2
    src, dst = torch.empty(half, dtype=torch.uint8, device=dev), torch.empty(half, dtype=torch.uint8, device=dev)

    def window(fn, iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / iters                                           # microseconds

    decode = lambda: train_input.decode(slot.staged_dev, staged.nbytes, staged.chunks, length, dim, out, ws, args.device)   # noqa: E731
    copy = lambda: dst.copy_(src)                                                         # noqa: E731
    window(decode, 20), window(copy, 20)
    rounds = [{"decode_us": window(decode, args.kernel_iters), "copy_us": window(copy, args.kernel_iters)} for _ in range(args.rounds)]
    kernel = median_rounds(rounds)
    # ---- steps per second
    weights = train.fresh_weights(params, dim, args.speakers, 0, channels=args.channels)
    head = train.build_trainer(params, weights, args.speakers, args.device, 0, "batch")
    resident = parent_batch(plan[0])
    offsets = np.arange(n + 1, dtype=np.int64) * length
    lr = 0.01

    def run_resident():
        for batch in plan[:args.steps]:
            head.step(resident, offsets, batch.labels, lr)

    def run_parent():
        for batch in plan[:args.steps]:
            head.step(parent_batch(batch), offsets, batch.labels, lr)

    def run_loader(prefetch):
        ld = train_input.Loader(data, spklist, params, 0, dim, args.device, prefetch=prefetch)

        def go():
            for feats, off, labels, _ in ld.batches(plan[:args.steps]):
                head.step(feats, off, labels, lr)
        return go

    variants = [("resident_steps_per_s", run_resident), ("parent_steps_per_s", run_parent),
                ("prefetch0_steps_per_s", run_loader(0)), ("prefetch2_steps_per_s", run_loader(2))]
    for _, fn in variants:
        fn()                                                                              # warm-up
    sync()
    rounds = []
    for _ in range(args.rounds):
        r = {}
        for name, fn in variants:
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            r[name] = args.steps / (time.perf_counter() - t0)
        rounds.append(r)
    steps = median_rounds(rounds)
    result = dict(utts=args.utts, segments=n, frames=length, dim=dim, batches=args.batches, steps=args.steps, rounds=args.rounds,
                  staged_bytes=staged.nbytes, kernel_in_bytes=in_bytes, kernel_out_bytes=out_bytes, same_bits=same,
                  kernel_gb_per_s=(in_bytes + out_bytes) / kernel["decode_us"] * 1e-3,
                  copy_gb_per_s=2 * half / kernel["copy_us"] * 1e-3, **per_batch, **kernel, **steps)
    print("per batch of %d x %d x %d: parent %.2f ms, new %.2f ms (staging alone %.2f ms); same bits: %s"
          % (n, length, dim, per_batch["parent_ms"], per_batch["new_ms"], per_batch["stage_ms"], same))
    print("decode kernel %.1f us (%.0f GB/s), device copy of the same bytes %.1f us (%.0f GB/s)"
          % (kernel["decode_us"], result["kernel_gb_per_s"], kernel["copy_us"], result["copy_gb_per_s"]))
    print("steps per second: resident batch %.1f, parent path %.1f, loader prefetch 0 %.1f, prefetch 2 %.1f"
          % (steps["resident_steps_per_s"], steps["parent_steps_per_s"], steps["prefetch0_steps_per_s"], steps["prefetch2_steps_per_s"]))
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
