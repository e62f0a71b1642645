"""A torch float64 model of the stack tf_kaldi_speaker_amd/att_train.py trains: frame layers (conv1d of any width) -> the key
and value networks on the endpoints att_key_input / att_value_input -> self-attentive pooling (the einsum formulation of
model/pooling.py:150-218) -> segment layers -> softmax head.  It is tests/test_gpu_bn_train.TorchStack with the pooling stage
replaced: batch norm in inference or training mode, the running statistics R kept across calls, the biased variance for every
attention layer (rank-2 kernels)."""
import numpy as np

import ref_att_pool as ra
from test_gpu_bn_train import HEAD_B, HEAD_K, TorchStack


def torch_att(cfg, key, value, query):
    """model/pooling.py:150-218 on one utterance (a batch of 1) -> pooled [2 P]; the floor mask enters as a constant."""
    import torch
    n, H = key.shape[0], cfg.H
    v = value[None].reshape(1, n, H, cfg.dv).permute(0, 2, 1, 3) if cfg.split_v else value[None, None]
    k = key[None].reshape(1, n, H, cfg.dq).permute(0, 2, 1, 3) if cfg.split_k else key[None, None]
    qk = torch.einsum("bhld,hd->blh" if cfg.split_k else "bmld,hd->blh", k, query) * cfg.scale
    w = torch.softmax(qk.transpose(1, 2), dim=-1)
    mean = torch.einsum("bhld,bhl->bhd" if cfg.split_v else "bmld,bhl->bhd", v, w)
    var = torch.einsum("bhld,bhl->bhd", (v - mean[:, :, None, :]) ** 2, w)
    mean, var = mean.reshape(1, -1), var.reshape(1, -1)
    mask = (var <= ra.FLOOR).to(torch.float64).detach()
    var = (1.0 - mask) * var + mask * ra.FLOOR
    return torch.cat([mean, torch.sqrt(var)], dim=1)[0]


class AttTorchStack(TorchStack):
    def __init__(self, trainer, weights, bessel):
        """From an att_train trainer: its specs, the nodes its attention reads (-1: the trainer's input) and the flags."""
        d = trainer.params.dict
        bessel = dict(bessel, **{s.kernel: False for s in trainer.att_specs})
        TorchStack.__init__(self, trainer.frame_specs, trainer.tail.specs, weights, bessel)
        import torch
        for spec in trainer.att_specs:
            if spec.bn:
                for s in ("moving_mean", "moving_variance"):
                    self.R[spec.bn + "/" + s] = torch.tensor(np.asarray(weights[spec.bn + "/" + s], dtype=np.float64))
        self.key_specs, self.value_specs, self.query = trainer.key_specs, trainer.value_specs, trainer.query_name
        self.key_node, self.value_node = trainer.key_node, trainer.value_node
        self.flags = (bool(d.get("att_split_key")), bool(d.get("att_split_value")), bool(d.get("att_use_scale")))

    def run(self, variables, x, offsets, labels, train):
        """-> (output endpoint, name -> gradient in TensorFlow shapes, name of a bias -> column sums of |gz| of its layer)."""
        torch = self.torch
        P = {k: torch.tensor(np.asarray(v, dtype=np.float64), requires_grad=True) for k, v in variables.items()}
        h, off, zs = torch.tensor(np.asarray(x, dtype=np.float64)), [int(o) for o in offsets], {}
        nodes = {-1: (h, off)}
        for j, spec in enumerate(self.frame_specs):
            k = P[spec.kernel]
            k3 = k[0] if k.dim() == 4 else k if k.dim() == 3 else k[None]                       # [W, C, N]
            w = k3.permute(2, 1, 0)
            outs = [torch.nn.functional.conv1d(h[off[u]:off[u + 1]].t()[None], w, P[spec.bias])[0].t() for u in range(len(off) - 1)]
            z = torch.cat(outs, dim=0)
            z.retain_grad()
            zs[spec.bias] = z
            off = [0] + [int(o) for o in np.cumsum([o.shape[0] for o in outs])]
            h = self._act(self._bn(z, spec, P, train), spec.act)
            nodes[j] = (h, off)

        def dense(h, specs):
            for spec in specs:
                z = h @ P[spec.kernel] + P[spec.bias]
                z.retain_grad()
                zs[spec.bias] = z
                h = self._act(self._bn(z, spec, P, train) if spec.bn else z, spec.act)
            return h

        (key, off), value = nodes[self.key_node], nodes[self.value_node][0]
        key, value = dense(key, self.key_specs), dense(value, self.value_specs)
        q = P[self.query]
        H, dq = int(q.shape[0]), int(q.shape[1])
        dv = int(value.shape[1]) // H if self.flags[1] else int(value.shape[1])
        cfg = ra.Cfg(H, dq, dv, *self.flags)
        h = torch.stack([torch_att(cfg, key[off[u]:off[u + 1]], value[off[u]:off[u + 1]], q) for u in range(len(off) - 1)])
        out = dense(h, self.seg_specs)
        if labels is None:
            return out.detach().numpy(), None, None
        logits = out @ P[HEAD_K] + P[HEAD_B]
        torch.nn.functional.cross_entropy(logits, torch.tensor(np.asarray(labels, dtype=np.int64))).backward()
        return (out.detach().numpy(), {k: p.grad.numpy() for k, p in P.items() if p.grad is not None},
                {k: z.grad.abs().sum(0).numpy() for k, z in zs.items()})
