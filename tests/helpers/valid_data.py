"""A small Kaldi data directory for the validation tests: feats.ark / feats.scp, spk2utt, utt2num_frames and a spklist."""
import os

import numpy as np

from tf_kaldi_speaker_amd import kaldi_io


def make_data_dir(tmp, spk_utts, lengths, dim=5, spklist=None, seed=0):
    """spk_utts: [(speaker, [utt, ...])] in feats.scp order; lengths: {utt: frames} -> (data dir, spklist path, {utt: matrix})."""
    rs = np.random.RandomState(seed)
    data = os.path.join(str(tmp), "data")
    os.makedirs(data, exist_ok=True)
    mats, scp = {}, []
    ark = os.path.join(data, "feats.ark")
    with open(ark, "wb") as f:
        for spk, utts in spk_utts:
            for u in utts:
                mats[u] = rs.standard_normal((lengths[u], dim)).astype(np.float32)
                scp.append("%s %s:%d\n" % (u, ark, f.tell() + len(u) + 1))
                kaldi_io.write_mat(f, mats[u], key=u)
    with open(os.path.join(data, "feats.scp"), "w") as f:
        f.writelines(scp)
    with open(os.path.join(data, "spk2utt"), "w") as f:
        for spk, utts in spk_utts:
            f.write("%s %s\n" % (spk, " ".join(utts)))
    with open(os.path.join(data, "utt2num_frames"), "w") as f:
        for u, t in lengths.items():
            f.write("%s %d\n" % (u, t))
    spklist_path = os.path.join(str(tmp), "spklist")
    with open(spklist_path, "w") as f:
        for spk, idx in (spklist or [(s, i) for i, (s, _) in enumerate(spk_utts)]):
            f.write("%s %d\n" % (spk, idx))
    return data, spklist_path, mats
