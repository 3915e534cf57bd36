"""CPU emulation of the fused kernel's "f16" arithmetic (PNR_PREC_F16): a twin of
``oracle.ref_cpu.resnetfc_forward`` in which every 512 -> 512 ``fc_0`` / ``fc_1`` is computed
as the kernel computes it:

* ``eW = scale_exp(max |W|)`` per layer and ``e = scale_exp(max |x|)`` per row of the
  layer's input (a point, or a (view, point) before the combine layer), the kernel's
  power-of-two scales (``scale_exp`` in csrc/mlp.hip: max * 2^e < 2^14, clamped to [-64, 40],
  0 for a zero / non-finite maximum);
* ``W 2^eW`` and ``relu(x) 2^e`` each rounded once to fp16 (round to nearest even);
* the products accumulated exactly (float64; every product of two fp16 values is exact in
  fp32, the kernel's fp32 accumulation adds its usual reassociation noise);
* the scales undone exactly and the fp32 bias added.

What the kernel leaves alone is left alone here: ``lin_in`` (the kernel keeps the two-part
f16x3 arithmetic there, fp32-level), the ``lin_z`` contribution (fp32 projected latent), the
multi-view mean and ``lin_out`` (fp32 head).

Install with ``monkeypatch.setattr(ref_cpu, "resnetfc_forward", f16_emul.resnetfc_forward)``:
``ref_cpu.pixelnerf_forward``, ``ref_cpu.render`` and ``parity.fine_pass_at`` then run on it
unchanged.  ``ROUND = False`` switches the fp16 roundings off: the twin then runs the same scaled graph
in the oracle's own fp32 arithmetic and equals the oracle within 1e-6."""
import torch
import torch.nn.functional as F

from oracle import ref_cpu

ROUND = True   # tests flip this to check the twin against the oracle


def scale_exp(m):
    """csrc/mlp.hip scale_exp on a tensor of maxima: int64 exponents."""
    m = m.detach().double()
    ok = (m > 0) & (m < 3.0e38)
    _, ex = torch.frexp(torch.where(ok, m, torch.ones_like(m)))   # m = f 2^ex, f in [0.5, 1)
    e = (14 - ex.long()).clamp(-64, 40)
    return torch.where(ok, e, torch.zeros_like(e))


def _f16(t):
    """fp64 -> fp16 (RNE) -> fp64.  The scaled operands stay below 2^14: no overflow."""
    return t.to(torch.float16).double() if ROUND else t


def linear_f16(x, w, b):
    """One 512 -> 512 layer in the kernel's single-product fp16 arithmetic.  x (N, 512) fp32."""
    ew = scale_exp(w.abs().max())
    e = scale_exp(x.abs().amax(-1))                      # (N,)
    if not ROUND:
        # the roundings off: the same scaled graph in the oracle's own arithmetic (fp32 F.linear;
        # the power-of-two scales are exact), so what is left to differ from the oracle is the
        # twin's structure and nothing else
        # (the bias enters at the products' scale, as the kernel's accumulators take it: one
        # F.linear per distinct row exponent)
        y = torch.empty(x.shape[0], w.shape[0])
        wsc = torch.ldexp(w, ew)
        for ev in torch.unique(e).tolist():
            rows = e == ev
            t = F.linear(torch.ldexp(x[rows], torch.tensor(ev)), wsc, torch.ldexp(b, torch.tensor(ev) + ew))
            y[rows] = torch.ldexp(t, -(torch.tensor(ev) + ew))
        return y
    ws = _f16(torch.ldexp(w.double(), ew))
    xs = _f16(torch.ldexp(x.double(), e.unsqueeze(-1)))
    y = torch.ldexp(xs @ ws.t(), -(e + ew).unsqueeze(-1))
    return (y + b.double()).float()


def resnetfc_forward(sd, prefix, zx, d_latent, n_blocks, combine_layer, inner_dims, relu=None):
    """``ref_cpu.resnetfc_forward`` with fc_0 / fc_1 of every block in the f16 arithmetic."""
    if relu is None:
        def relu(t, site):
            return torch.relu(t)

    def lin(name, t):
        return F.linear(t, sd[prefix + name + ".weight"], sd[prefix + name + ".bias"])

    def lin_h(name, t):
        w, b = sd[prefix + name + ".weight"], sd[prefix + name + ".bias"]
        if w.shape[0] != 512 or w.shape[1] != 512:       # only the 512-wide layers change
            return F.linear(t, w, b)
        shape = t.shape
        return linear_f16(t.reshape(-1, shape[-1]), w, b).reshape(*shape[:-1], w.shape[0])

    z = zx[..., :d_latent]
    x = zx[..., d_latent:]
    x = lin("lin_in", x)
    for blk in range(n_blocks):
        if blk == combine_layer:
            x = ref_cpu.combine_interleaved(x, inner_dims)
        if d_latent > 0 and blk < combine_layer:
            x = x + lin("lin_z.%d" % blk, z)
        net = lin_h("blocks.%d.fc_0" % blk, relu(x, ("x", blk)))
        dx = lin_h("blocks.%d.fc_1" % blk, relu(net, ("h", blk)))
        x = x + dx
    return lin("lin_out", relu(x, ("xf", n_blocks)))


def install(monkeypatch):
    monkeypatch.setattr(ref_cpu, "resnetfc_forward", resnetfc_forward)


# the fp32 term of "bounded by the emulation" (tests/test_gpu_f16.py): |d| <= ATOL + RTOL |ref|
ATOL, RTOL = 5e-5, 1e-5
