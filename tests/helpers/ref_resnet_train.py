"""A torch model of the stack tf_kaldi_speaker_amd/resnet_train.py trains, in float64 (or float32, to stand in for the device in
the seed precondition): conv0_1, the residual blocks (per-utterance F.pad + F.conv2d with TensorFlow's 'same' placement), conv5,
dense1, dense2, statistics pooling, the two segment layers and the head.  The batch norm's mode is a switch: eval (the moving
statistics, constants) or training (the statistics of the batch over all bins of all frames, the gradient through them, and the
running statistics R moved as tf.layers.batch_normalization moves them: towards the Bessel-corrected variance where the batch
norm sees rank 4 -- every convolution and conv5 -- and towards the biased one for dense1, dense2 and the segment layers).

small_model() is the configuration of tests/test_gpu_resnet_train.py: width 4, resnet_blocks [2, 1, 1, 1], pooling 24, last layer
16, three utterances of 9, 14 and 11 frames of 40 bins."""
import numpy as np

import ref_grid as rgd

EPS = 1e-3
WIDTH, POOL, LAST, DIM = 4, 24, 16, 40
LENS = (9, 14, 11)
HEAD_K, HEAD_B = "softmax/output/kernel", "softmax/output/bias"


# The cases of tests/test_gpu_resnet_train.py: name -> (batch_norm mode, params on top of small_model's, weight seed, the seed
# precondition's ratio measured on the CPU: the smallest |h| of the float64 model over its layer's largest float32-to-float64
# difference, sign_margin() below).  A whole-stack comparison is only sound where no activation input changes sign between the two
# computations; the ratio must be at least 8 (the device's rounding order is not torch's).  The seeds were chosen among 3 .. 12
# by that ratio, on the CPU alone; tests/test_resnet_train_host.py asserts it for every case.  No sign changed in any of the 80
# (seed, case) pairs scanned; 62 976 activation inputs without the time stride, 38 752 with it.
SGD = dict(optimizer="sgd", weight_l2_regularizer=1e-2, clip_gradient=True, clip_gradient_norm=0.5)
NESTEROV = dict(optimizer="momentum", momentum=0.9, use_nesterov=True, weight_l2_regularizer=1e-3)
ADAM = dict(optimizer="adam", weight_l2_regularizer=0.0)
ANGULAR = dict(loss_func="angular_triplet_loss", margin=0.2, triplet_type="all", loss_type="additive_margin_softmax")
CASES = {
    "moving-sgd": ("moving", dict(SGD), 5, 31.7),
    "moving-nesterov-lrelu": ("moving", dict(NESTEROV, network_relu_type="lrelu"), 11, 16.7),
    "moving-adam-stride": ("moving", dict(ADAM, resnet_time_stride=True), 4, 79.2),
    "batch-sgd": ("batch", dict(SGD, batchnorm_momentum=0.5), 12, 17.7),
    "batch-nesterov-stride-lrelu": ("batch", dict(NESTEROV, batchnorm_momentum=0.5, resnet_time_stride=True, network_relu_type="lrelu"),
                                    8, 54.9),
    "moving-metric": ("moving", dict(NESTEROV, use_nesterov=False, **ANGULAR), 8, 42.3),
}
MARGIN = 8.0


def small_model(seed, **extra):
    """-> (params dict, weights, feats [sum(LENS), 40] float32, frame offsets): feature seed = weight seed + 100."""
    from tf_kaldi_speaker_amd import synth
    params = dict(synth.RESNET_PARAMS, resnet_blocks=[2, 1, 1, 1], num_nodes_pooling_layer=POOL, num_nodes_last_layer=LAST)
    params.update(extra)
    weights = synth.synth_resnet_weights(params, seed=seed, width=WIDTH)
    feats = np.concatenate(synth.synth_features(len(LENS), LENS, DIM, seed=seed + 100))
    return params, weights, feats, np.concatenate([[0], np.cumsum(LENS)]).astype(np.int64)


class TorchResNet(object):
    """run() evaluates the stack at the given variables; R (name -> tensor) holds the running statistics across calls."""

    def __init__(self, params, weights, momentum=0.99, dtype=None):
        import torch
        from tf_kaldi_speaker_amd import resnet_train, tail_train
        self.torch, self.dtype = torch, dtype or torch.float64
        self.momentum = float(momentum)
        self.blocks = resnet_train.block_plan(params)
        self.frame_specs = resnet_train.frame_variables(params)
        self.seg_specs = tuple(tail_train.segment_variables(params))
        self.R = {}
        for spec in self.frame_specs + self.seg_specs:
            if spec.bn:
                for s in ("moving_mean", "moving_variance"):
                    self.R[spec.bn + "/" + s] = torch.tensor(np.asarray(weights[spec.bn + "/" + s], dtype=np.float64), dtype=self.dtype)

    # ------------------------------------------------------------------------------------------ pieces
    def _bn(self, z, spec, P, train, bessel):
        torch = self.torch
        bn = torch.nn.functional.batch_norm
        mm, mv = self.R[spec.bn + "/moving_mean"], self.R[spec.bn + "/moving_variance"]
        g, b = P[spec.bn + "/gamma"], P[spec.bn + "/beta"]
        if not train:
            return bn(z, mm, mv, g, b, False, 0.0, EPS)
        if bessel:
            return bn(z, mm, mv, g, b, True, 1.0 - self.momentum, EPS)       # torch's running_var takes n / (n - 1)
        y = bn(z, None, None, g, b, True, 0.0, EPS)
        with torch.no_grad():                                                # the same update fed the biased variance
            mm += (z.mean(0) - mm) * (1.0 - self.momentum)
            mv += (z.var(0, unbiased=False) - mv) * (1.0 - self.momentum)
        return y

    def _act(self, h, act, name):
        torch = self.torch
        if act != 0:
            self.pre.append((name, h.detach().numpy().copy()))
        return h if act == 0 else torch.relu(h) if act == 1 else torch.nn.functional.leaky_relu(h, float(np.float32(0.2)))

    def _conv(self, x, lens, bins, spec, P):
        """x rows (utterance, frame, bin) [*, C] -> (z rows, output lens, output bins): per-utterance F.pad + F.conv2d."""
        Fn = self.torch.nn.functional
        kh, kw, st, sf = spec.window
        w = P[spec.kernel].permute(3, 2, 0, 1)
        C = x.shape[1]
        outs, olens, row, Fo = [], [], 0, rgd.same_pad(bins, kw, sf)[0]
        for L in lens:
            xu = x[row:row + L * bins].reshape(1, L, bins, C).permute(0, 3, 1, 2)
            row += L * bins
            (Lo, pt), (_, pf) = rgd.same_pad(L, kh, st), rgd.same_pad(bins, kw, sf)
            tt, tf = max((Lo - 1) * st + kh - L, 0), max((Fo - 1) * sf + kw - bins, 0)
            z = Fn.conv2d(Fn.pad(xu, (pf, tf - pf, pt, tt - pt)), w, None, stride=(st, sf))
            outs.append(z.permute(0, 2, 3, 1).reshape(Lo * Fo, -1))
            olens.append(Lo)
        return self.torch.cat(outs, dim=0), olens, Fo

    # ------------------------------------------------------------------------------------------ the stack
    def run(self, variables, feats, lens, labels, train, loss=None):
        """-> dict(out: the output endpoint, grads: name -> gradient in TensorFlow shapes (None without labels), gz_sums: name of a
        bias in front of a batch norm -> column sums of |gz| of its layer, pre: [(name, h)] of every activation's input).
        `loss(rows, labels)`, if given, stands in the head's place (the metric door)."""
        torch = self.torch
        P = {k: torch.tensor(np.asarray(v, dtype=np.float64), dtype=self.dtype, requires_grad=True) for k, v in variables.items()}
        self.pre = []
        specs = list(self.frame_specs)
        lens, bins = [int(n) for n in lens], int(np.shape(feats)[1])
        x = torch.tensor(np.asarray(feats, dtype=np.float64), dtype=self.dtype).reshape(-1, 1)
        zs = {}

        def layer(x, lens, bins, spec):
            z, olens, obins = self._conv(x, lens, bins, spec, P)
            return self._act(self._bn(z, spec, P, train, True), spec.act, spec.bn), olens, obins

        x, lens, bins = layer(x, lens, bins, specs[0])
        i = 1
        for b in self.blocks:
            a, alens, abins = layer(x, lens, bins, specs[i])
            p, _, _ = layer(a, alens, abins, specs[i + 1])
            q = layer(x, lens, bins, specs[i + 2])[0] if b.shortcut else x
            x, lens, bins = self._act(p + q, specs[i].act, b.name + "_join"), alens, abins
            i += 3 if b.shortcut else 2
        h = x.reshape(sum(lens), bins * x.shape[1])
        for spec in specs[i:]:
            k = P[spec.kernel]
            z = h @ k.reshape(-1, k.shape[-1]) + P[spec.bias]
            z.retain_grad()
            zs[spec.bias] = z
            h = self._act(self._bn(z, spec, P, train, k.dim() == 4), spec.act, spec.bn)
        off = np.concatenate([[0], np.cumsum(lens)])
        rows = []
        for u in range(len(lens)):
            xu = h[off[u]:off[u + 1]]
            m = xu.mean(0)
            v = ((xu - m) ** 2).mean(0)
            rows.append(torch.cat([m, torch.sqrt(torch.clamp(v, min=1e-12))]))
        h = torch.stack(rows)
        for spec in self.seg_specs:
            z = h @ P[spec.kernel] + P[spec.bias]
            z.retain_grad()
            zs[spec.bias] = z
            h = self._act(self._bn(z, spec, P, train, False) if spec.bn else z, spec.act, spec.kernel)
        out = h
        res = dict(out=out.detach().numpy(), grads=None, gz_sums=None, pre=self.pre, loss=None)
        if labels is None:
            return res
        if loss is not None:
            value = loss(out, torch.tensor(np.asarray(labels, dtype=np.int64)))
        else:
            logits = out @ P[HEAD_K] + P[HEAD_B]
            value = torch.nn.functional.cross_entropy(logits, torch.tensor(np.asarray(labels, dtype=np.int64)))
        value.backward()
        res.update(loss=float(value.detach()), grads={k: p.grad.numpy() for k, p in P.items() if p.grad is not None},
                   gz_sums={k: z.grad.abs().sum(0).numpy() for k, z in zs.items() if z.grad is not None})
        return res


def sign_margin(params, weights, feats, lens, train):
    """The seed precondition: the float64 model against the same model in float32 (standing in for the device) at the
    checkpoint's variables -> (the smallest over the activations of min |h| / max |h32 - h64|, the number of activation inputs,
    the number whose sign differs, the largest layer error over the layer's rms)."""
    import torch
    variables = {k: v for k, v in weights.items() if "moving" not in k}
    momentum = params.get("batchnorm_momentum", 0.99)
    a = TorchResNet(params, weights, momentum).run(variables, feats, lens, None, train)["pre"]
    b = TorchResNet(params, weights, momentum, torch.float32).run(variables, feats, lens, None, train)["pre"]
    ratio, count, flips, worst = np.inf, 0, 0, 0.0
    for (name, h64), (_, h32) in zip(a, b):
        err = float(np.max(np.abs(h32.astype(np.float64) - h64)))
        ratio = min(ratio, float(np.min(np.abs(h64))) / max(err, 1e-300))
        worst = max(worst, err / float(np.sqrt(np.mean(h64 ** 2))))
        count += h64.size
        flips += int(np.sum((h64 > 0) != (h32 > 0)))
    return ratio, count, flips, worst
