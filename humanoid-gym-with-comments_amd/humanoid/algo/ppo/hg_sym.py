"""The mirror-symmetry loss on the HIP kernels ``hg_mirror_rows`` / ``hg_sym_loss`` /
``hg_sym_loss_backward`` (csrc/hg_sym.hip).

The reference (ppo.py:197-202) mirrors a minibatch with a dense product ``obs_batch @
obs_perm_mat`` ([mb, 705] x [705, 705]: 24 GFLOP per minibatch at the bench's size, to move and
negate columns), runs the actor on it, mirrors the result back with ``@ act_perm_mat`` and takes
``(mu - m_mirror_act).pow(2).mean()``.  Both matrices have one +-1 per column, so here a table is
a device ``(perm int32, sign float32)`` pair: ``mirror_rows`` is the signed column gather (one
HBM-bound pass), and ``sym_loss`` an autograd Function of two forward launches that writes the
loss together with its gradients with respect to both actor outputs; the backward scales them by
the incoming gradient (skipped for a registered unit seed, as hg_loss).  Device tensors only.
"""
import ctypes

import torch

from humanoid import _native as N
from . import hg_loss


def device_table(permutation, device):
    """(perm int32, sign float32) device tensors of a reference-format signed-index table: source
    column ``int(abs(p))``, negative iff ``p < 0`` (index 0 is negated by a small negative entry)."""
    perm = torch.tensor([int(abs(p)) for p in permutation], dtype=torch.int32, device=device)
    sign = torch.tensor([-1.0 if p < 0 else 1.0 for p in permutation], dtype=torch.float32, device=device)
    return perm, sign


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def mirror_rows(x, perm, sign, out=None):
    """out[r, c] = sign[c] * x[r, perm[c]] for a float32 [rows, width] device tensor with unit
    column stride (a column-offset view is fine); ``out`` (same shape, unit column stride, not
    ``x``) is allocated when None."""
    if x.dim() != 2 or x.dtype != torch.float32 or not x.is_cuda or x.stride(1) != 1:
        raise RuntimeError("mirror_rows needs a float32 [rows, width] device tensor with unit column stride")
    rows, width = x.shape
    if perm.numel() != width or sign.numel() != width or perm.dtype != torch.int32 or sign.dtype != torch.float32:
        raise RuntimeError(f"mirror_rows: the table must be int32 / float32 [{width}]")
    if out is None:
        out = torch.empty(rows, width, dtype=torch.float32, device=x.device)
    elif out.shape != x.shape or out.dtype != torch.float32 or out.stride(1) != 1 or out.device != x.device:
        raise RuntimeError("mirror_rows: out must match x (float32, unit column stride)")
    rc = N.lib().hg_mirror_rows(x.data_ptr(), x.stride(0), out.data_ptr(), out.stride(0), rows, width,
                                perm.data_ptr(), sign.data_ptr(), _stream(x.device))
    if rc != 0:
        raise RuntimeError(f"hg_mirror_rows failed ({rc})")
    return out


class _SymLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mu, mu_mirror, perm, sign, coef, sym_out):
        for t in (mu, mu_mirror):
            if t.dim() != 2 or t.dtype != torch.float32 or not t.is_cuda or t.stride(1) != 1:
                raise RuntimeError("sym_loss needs float32 [rows, A] device tensors with unit column stride")
        rows, A = mu.shape
        if mu_mirror.shape != mu.shape or perm.numel() != A or sign.numel() != A:
            raise RuntimeError("sym_loss: shapes of mu, mu_mirror and the action table disagree")
        dev = mu.device
        L = N.lib()
        loss = torch.empty((), dtype=torch.float32, device=dev)
        sym = torch.empty((), dtype=torch.float32, device=dev) if sym_out is None else sym_out
        g_mu = torch.empty(rows, A, dtype=torch.float32, device=dev)
        g_mir = torch.empty(rows, A, dtype=torch.float32, device=dev)
        scratch = torch.empty(int(L.hg_sym_loss_scratch(rows, A)), dtype=torch.float64, device=dev)
        rc = L.hg_sym_loss(mu.data_ptr(), mu.stride(0), mu_mirror.data_ptr(), mu_mirror.stride(0), perm.data_ptr(),
                           sign.data_ptr(), rows, A, float(coef), loss.data_ptr(), sym.data_ptr(), g_mu.data_ptr(),
                           g_mir.data_ptr(), scratch.data_ptr(), _stream(dev))
        if rc != 0:
            raise RuntimeError(f"hg_sym_loss failed ({rc})")
        ctx.save_for_backward(g_mu, g_mir)
        ctx.set_materialize_grads(False)
        if sym_out is not None:
            return loss  # the unweighted mean went to the caller's buffer
        ctx.mark_non_differentiable(sym)
        return loss, sym

    @staticmethod
    def backward(ctx, g_loss, g_sym=None):
        g_mu, g_mir = ctx.saved_tensors
        if g_loss.data_ptr() in hg_loss.UNIT_SEEDS:
            # seeded by a registered constant 1.0: scaling by exactly 1.0 is the identity
            return g_mu, g_mir, None, None, None, None
        g_loss = g_loss.contiguous()
        rows, A = g_mu.shape
        rc = N.lib().hg_sym_loss_backward(g_loss.data_ptr(), rows, A, g_mu.data_ptr(), g_mir.data_ptr(),
                                          _stream(g_mu.device))
        if rc != 0:
            raise RuntimeError(f"hg_sym_loss_backward failed ({rc})")
        return g_mu, g_mir, None, None, None, None


def sym_loss(mu, mu_mirror, perm, sign, coef=1.0, sym_out=None):
    """(loss, sym) with sym = mean((mu - sign * mu_mirror[:, perm])^2) (detached) and loss = coef *
    sym, differentiable in ``mu`` and ``mu_mirror`` (ppo.py:200-202, 208).  With ``sym_out`` (a
    float32 [] / [1] device buffer) the mean is written there and only the loss is returned.
    ``(perm, sign)``: the action table (device_table), a permutation of the action columns."""
    return _SymLoss.apply(mu, mu_mirror, perm, sign, coef, sym_out)
