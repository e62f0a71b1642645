"""Throughput of the waveform front-end on one MI355X, in frames per second:
  gpu        MFCC + energy VAD on the device (csrc/mfcc.hip), waveforms already resident
  oracle     the float64 numpy restatement (tests/helpers/ref_mfcc.py) on one core, on a sample of the utterances
  end2end    wav samples on the host -> MFCC -> VAD -> sliding CMN + voiced-frame selection -> x-vector network
8192 utterances with lengths drawn from U[2 s, 10 s], voxceleb options.  Prints one JSON line; results are kept in
profiles/frontend.md beside the extractor's own rate.
  --fbank    adds, on the same utterances and in the same run, fbank (the options of tests/golden/fbank_v3.conf) + energy VAD
             decided on the kernel's side energy, and its float64 oracle (tests/helpers/ref_fbank.py) on one core;
             --skip-end2end leaves the network leg out.

    python tools/frontend_bench.py [--utts 8192] [--batch-utts 1024] [--precision f16f6] [--oracle-utts 16] [--fbank]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=8192)
    ap.add_argument("--batch-utts", type=int, default=1024)
    ap.add_argument("--oracle-utts", type=int, default=16)
    ap.add_argument("--precision", type=str, default="")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--fbank", action="store_true")
    ap.add_argument("--skip-end2end", action="store_true")
    args = ap.parse_args()
    import torch
    import ref_mfcc
    from tf_kaldi_speaker_amd import mfcc as M, synth
    from tf_kaldi_speaker_amd.frontend import cmn_select_packed
    from tf_kaldi_speaker_amd.params import Params
    from tf_kaldi_speaker_amd.trainer import Trainer
    fs = 16000
    rng = np.random.RandomState(0)
    lens = rng.randint(2 * fs, 10 * fs + 1, size=args.utts)
    # one 10 s pool of speech-like samples (harmonics with a slow loud / quiet envelope + noise); utterances are windows of it
    t = np.arange(20 * fs) / fs
    pool = sum(a * np.sin(2 * np.pi * f * t + p) for a, f, p in ((3000, 130, 0.1), (1800, 390, 1.0), (900, 910, 2.0), (500, 1560, 3.0)))
    pool = pool * (0.5 + 0.5 * np.sign(np.sin(2 * np.pi * 1.3 * t))) + rng.uniform(-30, 30, size=t.shape[0])
    pool = np.round(pool).astype(np.int16)
    starts = rng.randint(0, 10 * fs, size=args.utts)
    mopts = M.MfccOptions(**ref_mfcc.VOXCELEB)
    vopts = M.VadOptions(**ref_mfcc.VAD_VOXCELEB)
    mf = M.Mfcc(mopts, 0)
    batches = []
    for i in range(0, args.utts, args.batch_utts):
        parts = [pool[s:s + n] for s, n in zip(starts[i:i + args.batch_utts], lens[i:i + args.batch_utts])]
        batches.append((np.concatenate(parts), np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)))
    frames = sum(mopts.num_frames(int(n)) for n in lens)

    def front(dev_batches):
        for w, off in dev_batches:
            f, foff = mf.compute(w, off)
            M.vad_packed(f, foff, vopts)

    dev_batches = [(torch.from_numpy(w).cuda(), off) for w, off in batches]
    front(dev_batches[:1])
    torch.cuda.synchronize()
    best = 1e30
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        front(dev_batches)
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    gpu_fps = frames / best
    result = {}
    if args.fbank:
        import ref_fbank
        from tf_kaldi_speaker_amd import fbank as F
        fopts = F.FbankOptions.from_config(os.path.join(ROOT, "tests", "golden", "fbank_v3.conf"))
        fb = F.Fbank(fopts, 0)
        fframes = sum(fopts.num_frames(int(n)) for n in lens)

        def front_fbank(dev_batches):
            for w, off in dev_batches:
                _, foff, energy = fb.compute(w, off, energy=True)
                M.vad_packed(energy.view(-1, 1), foff, vopts)

        front_fbank(dev_batches[:1])
        torch.cuda.synchronize()
        fbest = 1e30
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            front_fbank(dev_batches)
            torch.cuda.synchronize()
            fbest = min(fbest, time.perf_counter() - t0)
        fb.close()
        t0 = time.perf_counter()
        or_frames = 0
        for s, n in zip(starts[:min(args.oracle_utts, args.utts)], lens[:args.oracle_utts]):
            f, e = ref_fbank.fbank(pool[s:s + n], ref_fbank.V3)
            ref_mfcc.vad(e[:, None], ref_mfcc.VAD_VOXCELEB)
            or_frames += f.shape[0]
        result.update({"fbank_frames": int(fframes), "gpu_fbank_vad_frames_per_s": fframes / fbest, "gpu_fbank_vad_s": fbest,
                       "fbank_oracle_one_core_frames_per_s": or_frames / (time.perf_counter() - t0)})
    del dev_batches

    n_or = min(args.oracle_utts, args.utts)
    t0 = time.perf_counter()
    or_frames = 0
    for s, n in zip(starts[:n_or], lens[:n_or]):
        f = ref_mfcc.mfcc(pool[s:s + n], ref_mfcc.VOXCELEB)
        ref_mfcc.vad(f, ref_mfcc.VAD_VOXCELEB)
        or_frames += f.shape[0]
    oracle_fps = or_frames / (time.perf_counter() - t0)

    result.update({"utts": int(args.utts), "frames": int(frames), "audio_hours": float(lens.sum() / fs / 3600.0),
                   "gpu_mfcc_vad_frames_per_s": gpu_fps, "gpu_mfcc_vad_s": best,
                   "oracle_one_core_frames_per_s": oracle_fps, "oracle_utts": int(n_or)})
    if args.skip_end2end:
        mf.close()
        print(json.dumps(result))
        return
    params = Params(**dict(synth.TDNN_STAT_PARAMS))
    tr = Trainer(params, None, 30, single_cpu=True, device=0, precision=args.precision or None)
    tr.build("predict")
    tr.load_weights(synth.synth_weights(params, 30, seed=0))

    def end2end():
        kept_frames = 0
        for w, off in batches:
            f, foff = mf.compute(torch.from_numpy(w).cuda(), off)
            vad = M.vad_packed(f, foff, vopts).cpu().numpy()
            sel, soff, kept = cmn_select_packed(f, foff, [vad[foff[i]:foff[i + 1]] for i in range(len(off) - 1)], cmn_window=300,
                                                min_frames=25)
            tr.predict_packed(sel, soff).cpu()
            kept_frames += int(soff[-1])
        return kept_frames
    end2end()
    best2, kept_frames = 1e30, 0
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        kept_frames = end2end()
        torch.cuda.synchronize()
        best2 = min(best2, time.perf_counter() - t0)
    tr.close()
    mf.close()
    result.update({"end2end_frames_per_s": frames / best2, "end2end_s": best2, "voiced_fraction": kept_frames / float(frames),
                   "precision": args.precision or "default"})
    print(json.dumps(result))


if __name__ == "__main__":
    main()
