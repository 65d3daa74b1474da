"""A plain functional restatement of the residual U-Net blocks (MONAI 0.5 semantics), for float64 references.

Built only from ``F.conv3d``, ``F.conv_transpose3d``, ``F.instance_norm``, ``F.prelu``, ``+`` and ``torch.cat``;
it shares no forward code with ``texbias.unet``.  ``sd`` is a dict of named parameters as ``named_parameters()``
of the matching module yields them (any dtype / device); ``prefix`` is that module's name inside ``sd`` ("" for
the module itself).

Every function returns ``(y, inter)``.  ``inter`` maps the name of each ``Convolution`` block (the prefix of its
``conv.weight`` / ``adn.A.weight``) to its intermediates, all with ``retain_grad()`` when they take part in
autograd: ``z`` the conv output, and for blocks with an ADN ``n`` the normalised tensor and ``a`` the PReLU
output.  After a backward pass ``inter[c]["a"].grad`` is the gradient at the PReLU output (the terms of the
scalar PReLU weight gradient are ``n * a.grad`` over ``n <= 0``) and ``inter[c]["z"].grad`` the terms of the
conv's bias gradient.
"""
import torch
import torch.nn.functional as F

EPS = 1e-5


def _k(prefix: str, name: str) -> str:
    return f"{prefix}.{name}" if prefix else name


def _keep(t: torch.Tensor) -> torch.Tensor:
    if t.requires_grad:
        t.retain_grad()
    return t


def _adn(sd, cp: str, z: torch.Tensor, rec: dict) -> torch.Tensor:
    n = _keep(F.instance_norm(z, eps=EPS))
    a = _keep(F.prelu(n, sd[_k(cp, "adn.A.weight")]))
    rec["n"], rec["a"] = n, a
    return a


def _convolution(sd, cp: str, x, stride: int, conv_only: bool, transposed: bool, inter: dict):
    """MONAI ``Convolution``: (transposed) conv, kernel k, padding (k - 1) / 2 -> InstanceNorm -> PReLU."""
    w, b = sd[_k(cp, "conv.weight")], sd.get(_k(cp, "conv.bias"))
    pad = (w.shape[2] - 1) // 2
    if transposed:
        z = F.conv_transpose3d(x, w, b, stride=stride, padding=pad, output_padding=stride - 1)
    else:
        z = F.conv3d(x, w, b, stride=stride, padding=pad)
    rec = inter[cp] = {"z": _keep(z)}
    return z if conv_only else _adn(sd, cp, z, rec)


def residual_unit(sd, prefix: str, x, stride: int, subunits: int = 2, last_conv_only: bool = False):
    """``ResidualUnit``: ``subunits`` Convolutions (the first strided) + the residual path, summed."""
    inter = {}
    y = x
    for i in range(subunits):
        y = _convolution(sd, _k(prefix, f"conv.unit{i}"), y, stride if i == 0 else 1,
                         last_conv_only and i == subunits - 1, False, inter)
    wr = sd.get(_k(prefix, "residual.weight"))
    if wr is not None:
        res = F.conv3d(x, wr, sd.get(_k(prefix, "residual.bias")), stride=stride, padding=(wr.shape[2] - 1) // 2)
    else:
        res = x
    return y + res, inter


def up_block(sd, prefix: str, x, top: bool):
    """ConvTranspose3d(3, stride 2, padding 1, output_padding 1) -> ADN, then an identity-residual unit of
    one Convolution (a bare conv when ``top``)."""
    inter = {}
    a = _convolution(sd, _k(prefix, "0"), x, 2, False, True, inter)
    y, sub = residual_unit(sd, _k(prefix, "1"), a, 1, subunits=1, last_conv_only=top)
    inter.update(sub)
    return y, inter


def unet(sd, prefix: str, x, depth: int, top: bool = True):
    """The recursive ``Sequential(down, SkipConnection(sub), up)`` with ``depth`` stride-2 levels; the
    innermost ``sub`` is a stride-1 ``ResidualUnit``."""
    d, inter = residual_unit(sd, _k(prefix, "0"), x, 2)
    sp = _k(prefix, "1.submodule")
    if depth > 1:
        s, sub = unet(sd, sp, d, depth - 1, top=False)
    else:
        s, sub = residual_unit(sd, sp, d, 1)
    inter.update(sub)
    y, sub = up_block(sd, _k(prefix, "2"), torch.cat([d, s], dim=1), top)
    inter.update(sub)
    return y, inter


def split_params(names, inter: dict):
    """Sort parameter names into the three tolerance classes: (scalars, zero_biases, tensors) -- scalar
    PReLU weights {name: block}, conv biases ahead of an ADN (true gradient 0) {name: block}, and the rest."""
    scalars, zero_b, tensors = {}, {}, []
    for n in names:
        if n.endswith(".adn.A.weight") or n == "adn.A.weight":
            scalars[n] = n[:-len("adn.A.weight")].rstrip(".")
        elif n.endswith("conv.bias") and "n" in inter.get(n[:-len("conv.bias")].rstrip("."), {}):
            zero_b[n] = n[:-len("conv.bias")].rstrip(".")
        else:
            tensors.append(n)
    return scalars, zero_b, tensors


def prelu_cond(rec: dict) -> float:
    """sum over n <= 0 of |n dy|: the size of the terms a scalar PReLU weight gradient sums."""
    return (rec["n"].detach().clamp(max=0) * rec["a"].grad).abs().sum().item()


def bias_cond(rec: dict) -> float:
    """sum |dz|: the size of the terms the bias gradient of the conv that produced z sums."""
    return rec["z"].grad.abs().sum().item()
