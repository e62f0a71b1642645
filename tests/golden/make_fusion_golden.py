#!/usr/bin/env python
"""Generate tests/golden/average_score_{a,b,out}.txt by running the REFERENCE's own score fusion in the build container (never
on the GPU box, never at test time):

  /root/reference/misc/utils/average_score.py score1 score2 score_average       s = (float(s1) + float(s2)) / 2, written %f

Only the two seeded input score files and the file the script wrote (data) are stored; no reference source travels.  The
scores are float32 values printed with %.9g, so float32 holds exactly what the files say and the only roundings between the
stored output and a float32 fusion are the %f quantum (5e-7) and the one rounding of the result to float32 (2^-25 |s|);
they span both signs and four decades, which makes each of the two the larger term somewhere.
usage: python tests/golden/make_fusion_golden.py   (needs /root/reference)
"""
import os
import subprocess
import sys

import numpy as np

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    rs = np.random.RandomState(20)
    n = 40
    a = (rs.standard_normal(n) * 10.0 ** rs.randint(-2, 2, n)).astype(np.float32)
    b = (rs.standard_normal(n) * 10.0 ** rs.randint(-2, 2, n)).astype(np.float32)
    keys = [("spk%02d" % (i % 7), "utt%03d" % i) for i in range(n)]
    paths = [os.path.join(HERE, "average_score_%s.txt" % x) for x in ("a", "b", "out")]
    for path, s in zip(paths, (a, b)):
        with open(path, "w") as f:
            f.write("".join("%s %s %.9g\n" % (k1, k2, v) for (k1, k2), v in zip(keys, s)))
    subprocess.check_call([sys.executable, os.path.join(REF, "misc", "utils", "average_score.py")] + paths)
    assert len(open(paths[2]).read().splitlines()) == n
    print("wrote", ", ".join(os.path.basename(p) for p in paths))


if __name__ == "__main__":
    main()
