"""Every kernel variant include/i8ie_hip.h names and three numbers the library does not know (4, 53, 99), set
process-wide through $I8IE_KERNEL_VARIANT: AlexNet at 125 and 260 images (its pooled conv layers at batch sizes where
the patch-stationary kernel folds the pool, and where a forced choice leaves the pool to a launch of its own) and
two_conv at 16 images, through the i8ie surface, logits bit for bit against the oracle with the qparams the child
calibrated.  Probe and dispatch decide from the same decode (i8ie_conv_tries), so no value may end in the
dispatcher's pool / re-biased-layout invariant.  One child process per value (the variable is read when a ctx is
created), one after another; the first child that dies by a signal ends the test."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMED = [0, 3, 5, 11, 12, 13, 50, 54, 70, 80, 81, 83, 84, 85]  # the I8IE_VARIANT_* of include/i8ie_hip.h
VALUES = NAMED + [4, 53, 99]  # (numbers the library does not know: all behave like 0)
CASES = [("alexnet", 125), ("alexnet", 260), ("two_conv", 16)]

CHILD = r'''
import json, sys
import numpy as np
root, out, cases = sys.argv[1], sys.argv[2], json.loads(sys.argv[3])
sys.path.insert(0, root)
import int8inferenceengine_amd  # noqa: F401
import i8ie
from int8inferenceengine_amd import workloads as wl
logits, qparams = {}, {}
for name, batch in cases:
    key = "%s_%d" % (name, batch)
    net = wl.calibrated(name, wl.synthetic_state_dict(name))
    logits[key] = net(i8ie.tensor(wl.synthetic_input(name, batch, seed=5))).numpy()
    qparams[key] = {a: [float(s), int(z)] for a, (s, z) in ((a, getattr(net, a).output_qparams()) for a in wl.layer_names(name))}
np.savez(out + ".npz", **logits)
with open(out + ".json", "w") as f:
    json.dump(qparams, f)
'''


def test_every_variant_matches_the_oracle(tmp_path):
    import pipeline
    from int8inferenceengine_amd import workloads as wl

    oracle = {}  # (case, qparams) -> logits: the children calibrate alike, so this is computed once per case

    def want(name, batch, qp):
        k = (name, batch, json.dumps(qp, sort_keys=True))
        if k not in oracle:
            sd = wl.synthetic_state_dict(name)
            x = wl.synthetic_input(name, batch, seed=5)
            oracle[k] = pipeline.forward(wl.NETWORKS[name], x, pipeline.quantize_layers(wl.NETWORKS[name], sd),
                                         {a: (s, z) for a, (s, z) in qp.items()})
        return oracle[k]

    failed = []
    for v in VALUES:
        out = str(tmp_path / ("v%d" % v))
        r = subprocess.run([sys.executable, "-c", CHILD, ROOT, out, json.dumps(CASES)], cwd=ROOT,
                           env=dict(os.environ, I8IE_KERNEL_VARIANT=str(v)), capture_output=True, text=True, timeout=600)
        if r.returncode < 0:
            pytest.fail("variant %d: child died by signal %d (no further children started)\n%s" % (v, -r.returncode, r.stderr[-3000:]))
        if r.returncode != 0:
            failed.append("variant %d: exit %d: %s" % (v, r.returncode, r.stderr.strip().splitlines()[-1] if r.stderr.strip() else ""))
            continue
        got = np.load(out + ".npz")
        with open(out + ".json") as f:
            qps = json.load(f)
        for name, batch in CASES:
            key = "%s_%d" % (name, batch)
            w = want(name, batch, qps[key])
            if got[key].shape != w.shape or not np.array_equal(got[key].view(np.uint32), w.view(np.uint32)):
                failed.append("variant %d: %s logits differ from the oracle" % (v, key))
    assert not failed, "\n".join(failed)
