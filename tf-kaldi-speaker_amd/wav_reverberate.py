"""wav-reverberate on the GPU, one file, Kaldi's spelling:

    python -m tf_kaldi_speaker_amd.wav_reverberate [--impulse-response=R] [--additive-signals=A,B --snrs=.. --start-times=..]
        [--shift-output=true] [--normalize-output=true] [--duration=0] [--volume=0] [-g GPU] in.wav out.wav

`-` is stdin / stdout.  Options, defaults and the rule are those of tf_kaldi_speaker_amd.augment (include/xvec_hip.h states
the rule).  **parity unpinned**."""
import logging
import shlex
import sys
import tempfile

from . import augment


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    gpu, rest, i = 0, [], 0
    while i < len(argv):
        if argv[i] in ("-g", "--gpu") and i + 1 < len(argv):
            gpu, i = int(argv[i + 1]), i + 2
        elif argv[i].startswith("--gpu="):
            gpu, i = int(argv[i].split("=", 1)[1]), i + 1
        elif argv[i] in ("-h", "--help"):
            print(__doc__)
            return 0
        else:
            rest.append(argv[i])
            i += 1
    pos = [k for k, a in enumerate(rest) if not a.startswith("--")]
    tmp = None
    try:
        if len(pos) < 2:
            raise ValueError("expected <input> <output>")
        out = rest[pos[-1]]
        rest[pos[-1]] = "-"
        if rest[pos[-2]] == "-":                    # stdin: through a temporary file, which the pipeline grammar can name
            tmp = tempfile.NamedTemporaryFile(suffix=".wav")
            tmp.write(sys.stdin.buffer.read())
            tmp.flush()
            rest[pos[-2]] = tmp.name
        line = "wav-reverberate " + " ".join(shlex.quote(a) for a in rest) + " |"
        augment.parse_command(line)                 # option errors before the device is touched
        import torch
        with torch.cuda.device(gpu):
            b = augment.BatchBuilder()
            b.add(line)
            r = b.run("cuda:%d" % gpu)
        augment.write_wav(out, int(b.utts[0]["sample_rate"]), r.out_i16.cpu().numpy())
    except (ValueError, OSError) as e:
        sys.exit("wav_reverberate: %s" % e)
    finally:
        if tmp is not None:
            tmp.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
