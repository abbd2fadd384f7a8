"""torch.autograd.Function wrappers around the gfx950 HIP kernels."""
import torch
from torch.amp import custom_bwd, custom_fwd
from torch.autograd.function import once_differentiable

from .dispatch import _load_ext


class _LayerNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, eps):
        ext = _load_ext()
        x = x.contiguous()
        y, mean, rstd = ext.layernorm_fwd(x, weight, bias, float(eps))
        ctx.save_for_backward(x, weight, mean, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        ext = _load_ext()
        x, weight, mean, rstd = ctx.saved_tensors
        dx, dw, db = ext.layernorm_bwd(dy.contiguous(), x, weight, mean, rstd)
        return dx, dw, db, None


def hip_layer_norm(x, weight, bias, eps=1e-5):
    return _LayerNormFn.apply(x, weight, bias, eps)


class _GegluFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ext = _load_ext()
        x = x.contiguous()
        ctx.save_for_backward(x)
        return ext.geglu_fwd(x)

    @staticmethod
    def backward(ctx, dy):
        ext = _load_ext()
        (x,) = ctx.saved_tensors
        return ext.geglu_bwd(dy.contiguous(), x)


def hip_geglu(x):
    return _GegluFn.apply(x)


def _dgrad(dy2, weight):
    """dX = dY @ W.  hipBLASLt wins this shape class today (measured
    2x the custom kernel on dgrad_ff1, profiles/r02_ffgemm_ab.log);
    revisit when the staging upgrade lands."""
    return dy2 @ weight


import os as _os

# AF2AMD_WGRAD_V1=1: the r02 atomic-drain kernel behind its r02 gate, and
# bias gradients as separate reductions (A/B switch for the r09 kernel)
_WGRAD_V1 = _os.environ.get("AF2AMD_WGRAD_V1", "0") == "1"

# largest dW (elements) the streaming kernel takes: the largest measured
_WGRAD_STREAM_MAX_MN = 2048 * 256
_WGRAD_V1_MAX_MN = 256 * 512


def _wgrad(dy2, x2, want_colsum=False):
    """dW = dY^T @ X, and with want_colsum (dW, colsum) where colsum is
    the fp32 column sum of dY out of the same pass when the kernel ran,
    else None.

    K >= 65536 with dW up to 2048 x 256 elements goes to the streaming
    split-K kernel (wgrad.hip): one pass over dY and X, partials folded
    in a fixed order, so dW is the same on every run.  That is every
    Linear weight gradient of the trunk; at batch 5 the kernel runs them
    in 0.03-0.48 ms against 0.28-0.89 ms of the library GEMM and
    0.16-2.46 ms of the r02 kernel (tools/wgrad_bench.py,
    profiles/r09_wgrad_ab.log).  Larger outputs are not measured and
    small K stays on the library GEMM.  AF2AMD_WGRAD_V1=1 restores the
    r02 kernel and its gate (M * N <= 256 * 512)."""
    M, N = dy2.shape[-1], x2.shape[-1]
    K = dy2.shape[0]
    dw = cs = None
    if (K >= 65536 and M % 8 == 0 and N % 8 == 0
            and dy2.dtype == torch.bfloat16):
        if _WGRAD_V1:
            if M * N <= _WGRAD_V1_MAX_MN:
                dw = _load_ext().wgrad_v1(dy2.contiguous(), x2.contiguous())
        elif M * N <= _WGRAD_STREAM_MAX_MN:
            ext = _load_ext()
            if want_colsum:
                dw, cs = ext.wgrad_colsum(dy2.contiguous(), x2.contiguous())
            else:
                dw = ext.wgrad(dy2.contiguous(), x2.contiguous())
    if dw is None:
        dw = dy2.t() @ x2
    return (dw, cs) if want_colsum else dw


_FORCE_CUSTOM_LINEAR_FWD = _os.environ.get(
    "AF2AMD_CUSTOM_LINEAR", "0") == "1"


class _LinearFn(torch.autograd.Function):
    """out = x @ W.T (+ bias) (+ residual).

    Forward runs hipBLASLt (measured faster than the custom GEMM on
    plain/residual shapes) unless AF2AMD_CUSTOM_LINEAR=1; the value of
    routing plain Linears through this Function is the BACKWARD: the
    split-K wgrad kernel takes the small-output/huge-K gradients that
    Tensile handles poorly, and hands back the bias gradient (the column
    sum of dY) from the same pass."""

    @staticmethod
    @custom_fwd(device_type='cuda', cast_inputs=torch.bfloat16)
    def forward(ctx, x, weight, bias, residual):
        x = x.contiguous()
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        ctx.has_resid = residual is not None
        if _FORCE_CUSTOM_LINEAR_FWD:
            ext = _load_ext()
            return ext.linear_fwd(
                x, weight.contiguous(),
                bias.contiguous() if bias is not None else None,
                residual.contiguous() if residual is not None else None)
        out = torch.nn.functional.linear(x, weight, bias)
        if residual is not None:
            out = out + residual
        return out

    @staticmethod
    @custom_bwd(device_type='cuda')
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        dy2 = dy.contiguous().reshape(-1, dy.shape[-1])
        x2 = x.reshape(-1, x.shape[-1])
        dx = dw = db = None
        need_db = ctx.has_bias and ctx.needs_input_grad[2]
        # dW before dX: the kernel's split-K partials are free again when
        # the (larger) dX is allocated
        if ctx.needs_input_grad[1] and need_db:
            dw, colsum = _wgrad(dy2, x2, want_colsum=True)
            if colsum is not None:
                db = colsum.to(dy2.dtype)
        elif ctx.needs_input_grad[1]:
            dw = _wgrad(dy2, x2)
        if need_db and db is None:
            db = dy2.sum(dim=0)
        if ctx.needs_input_grad[0]:
            dx = _dgrad(dy2, weight).view_as(x)
        dr = dy if ctx.has_resid else None
        return dx, dw, db, dr


def hip_linear(x, weight, bias=None, residual=None):
    return _LinearFn.apply(x, weight, bias, residual)


class _FF1GegluFn(torch.autograd.Function):
    """GEGLU(x @ W.T + bias): one fused GEMM writing the gated half-width
    output plus the raw pre-activation (backward needs it for the gelu
    grads — the same tensor today's unfused path stores as the Linear
    output)."""

    @staticmethod
    @custom_fwd(device_type='cuda', cast_inputs=torch.bfloat16)
    def forward(ctx, x, weight, bias):
        ext = _load_ext()
        x = x.contiguous()
        out, inter = ext.ff1_geglu_fwd(
            x, weight.contiguous(),
            bias.contiguous() if bias is not None else None)
        ctx.save_for_backward(x, weight, inter)
        ctx.has_bias = bias is not None
        return out

    @staticmethod
    @custom_bwd(device_type='cuda')
    def backward(ctx, dy):
        ext = _load_ext()
        x, weight, inter = ctx.saved_tensors
        need_db = ctx.has_bias and ctx.needs_input_grad[2]
        # the bias gradient is the column sum of di: the kernel that
        # writes di forms it in the same pass where it covers the width
        db_sum = None
        if (need_db and inter.dtype == torch.bfloat16
                and inter.shape[-1] % 16 == 0
                and inter.shape[-1] // 2 <= ext.geglu_bwd_colsum_max_h()):
            di, db_sum = ext.geglu_bwd_colsum(dy.contiguous(), inter)
        else:
            di = ext.geglu_bwd(dy.contiguous(), inter)  # pre-act grad
        di2 = di.reshape(-1, di.shape[-1])
        x2 = x.reshape(-1, x.shape[-1])
        dx = dw = db = None
        if ctx.needs_input_grad[1]:
            dw = _wgrad(di2, x2)   # before dX, as in _LinearFn
        if ctx.needs_input_grad[0]:
            dx = _dgrad(di2, weight).view_as(x)
        if need_db:
            db = db_sum.to(di2.dtype) if db_sum is not None \
                else di2.sum(dim=0)
        return dx, dw, db


def hip_ff1_geglu(x, weight, bias=None):
    return _FF1GegluFn.apply(x, weight, bias)


def _attn_fwd(ext, ctx, q, k, v, bias, mask, bias_repeat, scale,
              dropout_p, rng_state, **kw):
    """ext.attn_fwd with or without attention-probability dropout.
    Returns (out, lse, rng_state); rng_state is the int64[2] device
    tensor (seed, offset) the kernel used — the caller's, or the one the
    forward drew from the default generator — and None without dropout.
    It is kept on ctx for the backward (a plain attribute: it is neither
    an input nor an output of the graph the Function records)."""
    ctx.dropout_p = dropout_p
    if dropout_p > 0.:
        out, lse, rng_state = ext.attn_fwd(
            q, k, v, bias, mask, bias_repeat, scale, dropout_p=dropout_p,
            rng_state=rng_state, **kw)
    else:
        out, lse = ext.attn_fwd(q, k, v, bias, mask, bias_repeat, scale, **kw)
        rng_state = None
    ctx.rng_state = rng_state
    return out, lse, rng_state


def _drop_kw(ctx):
    if ctx.dropout_p > 0.:
        return dict(dropout_p=ctx.dropout_p, rng_state=ctx.rng_state)
    return {}


def _fn_result(ctx, out, rng_state, want_state):
    """(out, rng_state) when the caller asked for the state, else out."""
    if not want_state:
        return out
    assert rng_state is not None, "return_rng_state needs dropout_p > 0"
    ctx.mark_non_differentiable(rng_state)
    return out, rng_state


class _AttentionFn(torch.autograd.Function):
    """Fused flash attention (bf16, head dim 64) with broadcast pair bias.

    bias has shape (B // bias_repeat, h, Lq, Lk); consecutive groups of
    `bias_repeat` batch entries share a bias slice (the axial-attention
    fold — never materialized).  dropout_p > 0 drops attention
    probabilities inside the kernels (ops/hip/attn_dropout.h).
    """

    @staticmethod
    def forward(ctx, q, k, v, bias, mask, bias_repeat, scale,
                dropout_p=0., rng_state=None, want_state=False):
        ext = _load_ext()
        # q/k/v are consumed through their strides (no permute copies);
        # only the innermost head-dim must be dense
        bias_c = bias.contiguous() if bias is not None else None
        mask_c = mask.contiguous() if mask is not None else None
        out, lse, rng_state = _attn_fwd(ext, ctx, q, k, v, bias_c, mask_c,
                                        bias_repeat, scale, dropout_p,
                                        rng_state)
        ctx.save_for_backward(q, k, v, out, lse,
                              *( [bias_c] if bias_c is not None else [] ))
        ctx.has_bias = bias_c is not None
        ctx.mask = mask_c
        ctx.bias_repeat = bias_repeat
        ctx.scale = scale
        ctx.bias_requires_grad = bias is not None and bias.requires_grad
        return _fn_result(ctx, out, rng_state, want_state)

    @staticmethod
    def backward(ctx, dout, *_):
        ext = _load_ext()
        saved = ctx.saved_tensors
        q, k, v, out, lse = saved[:5]
        bias = saved[5] if ctx.has_bias else None
        need_dbias = ctx.bias_requires_grad
        rets = ext.attn_bwd(dout, q, k, v, out, lse, bias,
                            ctx.mask, ctx.bias_repeat, ctx.scale, need_dbias,
                            **_drop_kw(ctx))
        dq, dk, dv = rets[:3]
        dbias = rets[3].to(bias.dtype) if need_dbias else None
        return dq, dk, dv, dbias, None, None, None, None, None, None


def hip_attention_core(q, k, v, bias=None, mask=None, context_mask=None,
                       tie_dim=None, bias_repeat=1, scale=None,
                       dropout_p=0., rng_state=None, return_rng_state=False):
    """dropout_p > 0 drops attention probabilities in the kernels; the
    mask is a function of `rng_state` (int64[2] device tensor: seed,
    offset), drawn from the default generator when not given.
    return_rng_state=True returns (out, rng_state)."""
    key_mask = context_mask if context_mask is not None else mask
    if key_mask is not None:
        key_mask = key_mask.to(torch.uint8)
        if key_mask.shape[0] != q.shape[0]:
            # the kernel indexes mask[batch * Lk + j]: broadcast masks
            # (e.g. the (1, Lk) cross-attention default) expand here
            key_mask = key_mask.expand(q.shape[0], -1).contiguous()
    dh = q.shape[-1]
    if scale is None:
        scale = dh ** -0.5
    if dh < 64:
        # narrow heads run on the 64-wide MFMA tile via zero padding:
        # QK^T and the real output channels of PV are invariant to
        # zero-padded channels, and autograd differentiates the
        # pad/slice pair (scale already fixed to the REAL head dim)
        pad = 64 - dh
        q, k, v = (torch.nn.functional.pad(t, (0, pad)) for t in (q, k, v))
        out = hip_attention_core(q, k, v, bias=bias, mask=None,
                                 context_mask=key_mask, tie_dim=tie_dim,
                                 bias_repeat=bias_repeat, scale=scale,
                                 dropout_p=dropout_p, rng_state=rng_state,
                                 return_rng_state=return_rng_state)
        if return_rng_state:
            return out[0][..., :dh], out[1]
        return out[..., :dh]
    if tie_dim is not None:
        return _AttentionTiedFn.apply(q, k, v, bias, key_mask, tie_dim,
                                      bias_repeat, scale, dropout_p,
                                      rng_state, return_rng_state)
    return _AttentionFn.apply(q, k, v, bias, key_mask, bias_repeat, scale,
                              dropout_p, rng_state, return_rng_state)


class _AttentionTiedFn(torch.autograd.Function):
    """Tied-query ("global column", reference alphafold2.py:142-151)
    attention on the fused kernels: queries are MEANED over groups of
    `tie_dim` consecutive batch entries and the group-mean query attends
    to each entry's own keys/values.  K2 in SURVEY.md §2.17.

    Runs as standard attention with the group-mean query replicated
    across the group (one bf16 copy); backward group-sums dq_exp and
    divides by tie_dim (the mean+broadcast chain rule), so dq matches
    plain autograd exactly.
    """

    @staticmethod
    def forward(ctx, q, k, v, bias, mask, tie_dim, bias_repeat, scale,
                dropout_p=0., rng_state=None, want_state=False):
        ext = _load_ext()
        Bh = q.shape[0]
        b = Bh // tie_dim
        # group-mean query, consumed via the kernels' q_repeat divisor —
        # the tie_dim-fold replication is never materialized
        qm = q.reshape(b, tie_dim, *q.shape[1:]).mean(dim=1).contiguous()
        bias_c = bias.contiguous() if bias is not None else None
        mask_c = mask.contiguous() if mask is not None else None
        # the dropout mask is indexed by the K/V batch entry, so every
        # member of a tie group draws its own (as the eager composition)
        out, lse, rng_state = _attn_fwd(ext, ctx, qm, k, v, bias_c, mask_c,
                                        bias_repeat, scale, dropout_p,
                                        rng_state, q_repeat=tie_dim)
        ctx.save_for_backward(qm, k, v, out, lse,
                              *([bias_c] if bias_c is not None else []))
        ctx.has_bias = bias_c is not None
        ctx.mask = mask_c
        ctx.meta = (tie_dim, bias_repeat, scale)
        ctx.bias_requires_grad = bias is not None and bias.requires_grad
        return _fn_result(ctx, out, rng_state, want_state)

    @staticmethod
    def backward(ctx, dout, *_):
        ext = _load_ext()
        saved = ctx.saved_tensors
        qm, k, v, out, lse = saved[:5]
        bias = saved[5] if ctx.has_bias else None
        tie_dim, bias_repeat, scale = ctx.meta
        need_dbias = ctx.bias_requires_grad
        rets = ext.attn_bwd(dout, qm, k, v, out, lse, bias,
                            ctx.mask, bias_repeat, scale, need_dbias,
                            q_repeat=tie_dim, **_drop_kw(ctx))
        dq_exp, dk, dv = rets[:3]
        Bh = dq_exp.shape[0]
        b = Bh // tie_dim
        dq = dq_exp.reshape(b, tie_dim, *dq_exp.shape[1:]) \
                   .sum(dim=1, keepdim=True).div_(tie_dim) \
                   .expand(b, tie_dim, *dq_exp.shape[1:]) \
                   .reshape(Bh, *dq_exp.shape[1:])
        dbias = rets[3].to(bias.dtype) if need_dbias else None
        return dq, dk, dv, dbias, None, None, None, None, None, None, None


class _AttentionPackedFn(torch.autograd.Function):
    """Self-attention over a PACKED projection tensor (B, L, W) holding
    [q | k | v | ...] channel blocks of h*dh each.  The backward writes
    dq/dk/dv directly into slices of ONE grad buffer, so autograd never
    concatenates three per-slice gradients (the split-backward cat was
    ~5% of a training step)."""

    @staticmethod
    def forward(ctx, packed, heads, inner, bias, mask, bias_repeat, scale,
                dropout_p=0., rng_state=None, want_state=False):
        ext = _load_ext()
        B, L = packed.shape[0], packed.shape[1]
        dh = inner // heads

        def view(off):
            return packed.narrow(-1, off, inner)                 .view(B, L, heads, dh).permute(0, 2, 1, 3)

        q, k, v = view(0), view(inner), view(2 * inner)
        bias_c = bias.contiguous() if bias is not None else None
        mask_c = mask.contiguous() if mask is not None else None
        out, lse, rng_state = _attn_fwd(ext, ctx, q, k, v, bias_c, mask_c,
                                        bias_repeat, scale, dropout_p,
                                        rng_state)
        ctx.save_for_backward(packed, out, lse,
                              *([bias_c] if bias_c is not None else []))
        ctx.has_bias = bias_c is not None
        ctx.mask = mask_c
        ctx.meta = (heads, inner, bias_repeat, scale)
        ctx.bias_requires_grad = bias is not None and bias.requires_grad
        return _fn_result(ctx, out, rng_state, want_state)

    @staticmethod
    def backward(ctx, dout, *_):
        ext = _load_ext()
        saved = ctx.saved_tensors
        packed, out, lse = saved[:3]
        bias = saved[3] if ctx.has_bias else None
        heads, inner, bias_repeat, scale = ctx.meta
        B, L, W = packed.shape
        dh = inner // heads

        # dq/dk/dv slices are fully overwritten by the kernel; only the
        # remaining channels (the gate block) must start at zero — their
        # gradient arrives via the other autograd path and is summed
        dpacked = torch.empty_like(packed)
        if W > 3 * inner:
            dpacked.narrow(-1, 3 * inner, W - 3 * inner).zero_()

        def view(t, off):
            return t.narrow(-1, off, inner)                 .view(B, L, heads, dh).permute(0, 2, 1, 3)

        q, k, v = view(packed, 0), view(packed, inner), view(packed, 2 * inner)
        dq, dk, dv = (view(dpacked, 0), view(dpacked, inner),
                      view(dpacked, 2 * inner))
        need_dbias = ctx.bias_requires_grad
        rets = ext.attn_bwd(dout, q, k, v, out, lse, bias, ctx.mask,
                            bias_repeat, scale, need_dbias,
                            dq_out=dq, dk_out=dk, dv_out=dv,
                            **_drop_kw(ctx))
        dbias = rets[3].to(bias.dtype) if need_dbias else None
        return (dpacked, None, None, dbias, None, None, None, None, None,
                None)


def hip_attention_packed(packed, heads, inner, bias=None, mask=None,
                         bias_repeat=1, dropout_p=0., rng_state=None,
                         return_rng_state=False, gated_input=None):
    """gated_input=(x, w_cat, gate_bias) with packed=None runs projection,
    attention and output gate as one unit (_GatedAttentionUnitFn) and
    returns the gated (B, L, inner) output."""
    key_mask = mask.to(torch.uint8) if mask is not None else None
    scale = (inner // heads) ** -0.5
    if gated_input is not None:
        x, w_cat, gate_bias = gated_input
        return _GatedAttentionUnitFn.apply(x, w_cat, gate_bias, bias,
                                           key_mask, heads, bias_repeat,
                                           scale, dropout_p, rng_state,
                                           return_rng_state)
    return _AttentionPackedFn.apply(packed, heads, inner, bias, key_mask,
                                    bias_repeat, scale, dropout_p, rng_state,
                                    return_rng_state)


class _GatedAttentionUnitFn(torch.autograd.Function):
    """Gated self-attention as ONE autograd unit, projection included:

        fused = x @ w_cat.T + [0 | 0 | 0 | gate_bias]     # [q|k|v|gate]
        y     = attention(q, k, v) * sigmoid(gate)

    The forward issues the calls the separate path issues (the same
    F.linear, attn_fwd and gatemul_fwd on the same operands).  The value
    is the BACKWARD: `fused` has a single consumer, so one pass
    (attn_gate_bwd) writes dgate straight into the gate slice of the
    packed gradient and hands dO and delta to attn_bwd — no zero fills,
    no slice copy and no full-width add from autograd, no
    attn_delta_kernel — and the gating-bias gradient is that pass's
    column sum instead of a reduce over all four channel blocks."""

    @staticmethod
    @custom_fwd(device_type='cuda', cast_inputs=torch.bfloat16)
    def forward(ctx, x, w_cat, gate_bias, bias, mask, heads, bias_repeat,
                scale, dropout_p=0., rng_state=None, want_state=False):
        ext = _load_ext()
        B, L = x.shape[0], x.shape[1]
        inner = w_cat.shape[0] // 4
        dh = inner // heads
        bias_cat = torch.cat([gate_bias.new_zeros(3 * inner), gate_bias])
        fused = torch.nn.functional.linear(x, w_cat, bias_cat)

        def view(off):
            return fused.narrow(-1, off, inner) \
                .view(B, L, heads, dh).permute(0, 2, 1, 3)

        q, k, v = view(0), view(inner), view(2 * inner)
        bias_c = bias.contiguous() if bias is not None else None
        mask_c = mask.contiguous() if mask is not None else None
        out, lse, rng_state = _attn_fwd(ext, ctx, q, k, v, bias_c, mask_c,
                                        bias_repeat, scale, dropout_p,
                                        rng_state)
        # out is (B, h, L, dh) over (B, L, h, dh) memory: a free reshape
        y = ext.gatemul_fwd(out.permute(0, 2, 1, 3).reshape(B, L, inner),
                            fused.narrow(-1, 3 * inner, inner),
                            inner, fused.shape[-1], None)
        ctx.save_for_backward(x, w_cat, fused, out, lse,
                              *([bias_c] if bias_c is not None else []))
        ctx.has_bias = bias_c is not None
        ctx.mask = mask_c
        ctx.meta = (heads, inner, bias_repeat, scale)
        ctx.bias_requires_grad = bias is not None and bias.requires_grad
        ctx.gate_bias_dtype = gate_bias.dtype
        return _fn_result(ctx, y, rng_state, want_state)

    @staticmethod
    @custom_bwd(device_type='cuda')
    def backward(ctx, dy, *_):
        ext = _load_ext()
        saved = ctx.saved_tensors
        x, w_cat, fused, out, lse = saved[:5]
        bias = saved[5] if ctx.has_bias else None
        heads, inner, bias_repeat, scale = ctx.meta
        B, L, W = fused.shape
        dh = inner // heads
        need_dx, need_dw, need_dgb = ctx.needs_input_grad[:3]

        # every channel block is fully overwritten: no fill
        dpacked = torch.empty_like(fused)

        def view(t, off):
            return t.narrow(-1, off, inner) \
                .view(B, L, heads, dh).permute(0, 2, 1, 3)

        rets = ext.attn_gate_bwd(dy.contiguous(), out,
                                 fused.narrow(-1, 3 * inner, inner),
                                 dpacked.narrow(-1, 3 * inner, inner),
                                 need_dgb)
        d_o, delta = rets[:2]
        need_dbias = ctx.bias_requires_grad
        arets = ext.attn_bwd(d_o, view(fused, 0), view(fused, inner),
                             view(fused, 2 * inner), out, lse, bias, ctx.mask,
                             bias_repeat, scale, need_dbias,
                             dq_out=view(dpacked, 0),
                             dk_out=view(dpacked, inner),
                             dv_out=view(dpacked, 2 * inner),
                             delta=delta, **_drop_kw(ctx))
        dbias = arets[3].to(bias.dtype) if need_dbias else None

        # the two matmuls autograd runs for F.linear
        dp2 = dpacked.view(-1, W)
        dw = _wgrad(dp2, x.reshape(-1, x.shape[-1])) if need_dw else None
        dx = (dp2 @ w_cat).view_as(x) if need_dx else None
        dgb = rets[2].to(ctx.gate_bias_dtype) if need_dgb else None
        return (dx, dw, dgb, dbias, None, None, None, None, None, None,
                None)


def _uniform_row_stride(t):
    """Row stride (elements) if the tensor enumerates as (rows, C) with
    one uniform stride (e.g. a channel slice of a fused projection);
    None if the layout is irregular."""
    C = t.shape[-1]
    if t.stride(-1) != 1:
        return None
    if t.dim() == 1:
        return C
    rs = t.stride(-2)
    mult = t.shape[-2]
    for i in range(t.dim() - 3, -1, -1):
        if t.shape[i] != 1 and t.stride(i) != rs * mult:
            return None
        mult *= t.shape[i]
    return rs


class _GateMulFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, g, rowmask):
        ext = _load_ext()
        xs = _uniform_row_stride(x)
        gs = _uniform_row_stride(g)
        if xs is None:
            x = x.contiguous()
            xs = x.shape[-1]
        if gs is None:
            g = g.contiguous()
            gs = g.shape[-1]
        rm = rowmask.reshape(-1).to(torch.uint8).contiguous() \
            if rowmask is not None else None
        ctx.save_for_backward(x, g)
        ctx.strides = (xs, gs)
        ctx.rm = rm
        return ext.gatemul_fwd(x, g, xs, gs, rm)

    @staticmethod
    def backward(ctx, dy):
        ext = _load_ext()
        x, g = ctx.saved_tensors
        xs, gs = ctx.strides
        dx, dg = ext.gatemul_bwd(dy.contiguous(), x, g, xs, gs, ctx.rm)
        return dx, dg, None


def hip_gatemul(x, g, rowmask=None):
    return _GateMulFn.apply(x, g, rowmask)


def _pcg(A, B, M, N, K, a_m, a_k, b_n, b_k, alpha=1.0, variant=0):
    """Invoke the per-channel GEMM: C[b,m,n,d] = alpha * sum_k A*B where
    a_m/a_k (b_n/b_k) are the AXIS INDICES (1 or 2) of A (B) that play
    the output-m (output-n) and contraction roles.  variant picks the
    kernel for A/B runs and tests: 1 = scatter staging, 2 = wide stores,
    3 = full lines, 0 = the extension's default."""
    ext = _load_ext()
    D = A.shape[-1]
    Bb = A.shape[0]
    return ext.pcgemm(A, B, Bb, M, N, K, D,
                      A.stride(0), A.stride(a_m), A.stride(a_k),
                      B.stride(0), B.stride(b_n), B.stride(b_k), alpha,
                      variant)


def _pc_ok(*ts):
    for t in ts:
        if t.stride(-1) != 1 or t.shape[-1] % 8 != 0:
            return False
        if any(st % 8 != 0 for st in t.stride()[:-1]):
            return False
    return True


class _TriMixFn(torch.autograd.Function):
    """Triangle multiplicative mixing on the gfx950 per-channel GEMM.

    outgoing: C[i,j] = sum_k L[i,k] R[j,k]
    ingoing:  C[i,j] = sum_k L[k,j] R[k,i]
    """

    @staticmethod
    def forward(ctx, left, right, mix):
        n = left.shape[1]
        ctx.save_for_backward(left, right)
        ctx.mix = mix
        if mix == 'outgoing':
            return _pcg(left, right, n, n, n, 1, 2, 1, 2)
        return _pcg(right, left, n, n, n, 2, 1, 2, 1)

    @staticmethod
    def backward(ctx, dC):
        left, right = ctx.saved_tensors
        n = left.shape[1]
        dC = dC.contiguous()
        if ctx.mix == 'outgoing':
            # dL[i,k] = sum_j dC[i,j] R[j,k];  dR[j,k] = sum_i dC[i,j] L[i,k]
            dL = _pcg(dC, right, n, n, n, 1, 2, 2, 1)
            dR = _pcg(dC, left, n, n, n, 2, 1, 2, 1)
        else:
            # C[i,j] = sum_k L[k,j] R[k,i]
            # dL[k,j] = sum_i R[k,i] dC[i,j]; dR[k,i] = sum_j L[k,j] dC[i,j]
            dL = _pcg(right, dC, n, n, n, 1, 2, 2, 1)
            dR = _pcg(left, dC, n, n, n, 1, 2, 1, 2)
        return dL, dR, None


def hip_triangle_mix(left, right, mix):
    if not _pc_ok(left, right):
        from . import eager
        return eager.triangle_mix(left, right, mix)
    return _TriMixFn.apply(left.contiguous() if left.stride(-1) != 1 else left,
                           right, mix)


class _OuterSumFn(torch.autograd.Function):
    """sum_m L[b,m,i,d] R[b,m,j,d] -> (b,i,j,d), scaled by alpha."""

    @staticmethod
    def forward(ctx, left, right, alpha):
        b, m, n, d = left.shape
        ctx.save_for_backward(left, right)
        ctx.alpha = alpha
        return _pcg(left, right, n, n, m, 2, 1, 2, 1, alpha=alpha)

    @staticmethod
    def backward(ctx, dC):
        left, right = ctx.saved_tensors
        b, m, n, d = left.shape
        dC = dC.contiguous()
        # dL[m,i] = a * sum_j R[m,j] dC[i,j]; dR[m,j] = a * sum_i L[m,i] dC[i,j]
        dL = _pcg(right, dC, m, n, n, 1, 2, 1, 2, alpha=ctx.alpha)
        dR = _pcg(left, dC, m, n, n, 1, 2, 2, 1, alpha=ctx.alpha)
        return dL, dR, None


def hip_outer_product_mean(left, right, mask=None, eps=1e-5):
    """Reference-numerics outer-product mean on the per-channel GEMM
    (masked branch: sum_m / (m * (count + eps)) — see ops/eager.py)."""
    m = left.shape[1]
    if not _pc_ok(left, right):
        from . import eager
        return eager.outer_product_mean(left, right, mask=mask, eps=eps)
    if mask is not None:
        fmask = mask.to(left.dtype)
        left = left * fmask[..., None]
        right = right * fmask[..., None]
        outer_sum = _OuterSumFn.apply(left.contiguous(), right.contiguous(),
                                      1.0 / m)
        count = torch.einsum('b m i, b m j -> b i j', fmask, fmask)
        return outer_sum / (count[..., None] + eps)
    return _OuterSumFn.apply(left.contiguous(), right.contiguous(), 1.0 / m)


class _TriProjGatesFn(torch.autograd.Function):
    """TriangleMultiplicative's gated projections as ONE unit over the
    fused [left | right | lgate | rgate | ogate] projection (…, 5h):

        gated_left  = left  * sigmoid(lgate) * mask
        gated_right = right * sigmoid(rgate) * mask
        og          = ogate                       (passthrough slice)

    The forward reads strided slices (no copies, as before); the win is
    the BACKWARD: both gatemul gradients are written straight into
    slices of one packed d_fused buffer, so autograd never runs the
    5-way SplitBackward concatenation (~16 ms/step at batch 5)."""

    @staticmethod
    def forward(ctx, fused, hdim, rowmask):
        ext = _load_ext()
        C5 = fused.shape[-1]
        assert C5 == 5 * hdim
        fused = fused.contiguous()
        rm = rowmask.reshape(-1).to(torch.uint8).contiguous() \
            if rowmask is not None else None

        def sl(i):
            return fused.narrow(-1, i * hdim, hdim)

        left = ext.gatemul_fwd(sl(0), sl(2), C5, C5, rm)
        right = ext.gatemul_fwd(sl(1), sl(3), C5, C5, rm)
        ctx.save_for_backward(fused)
        ctx.hdim = hdim
        ctx.rm = rm
        return left, right, sl(4)

    @staticmethod
    def backward(ctx, d_left, d_right, d_og):
        ext = _load_ext()
        (fused,) = ctx.saved_tensors
        h = ctx.hdim
        C5 = fused.shape[-1]
        d_fused = torch.empty_like(fused)

        def sl(t, i):
            return t.narrow(-1, i * h, h)

        def bwd_pair(dy, xi, gi):
            # an output can be unused downstream (None grad): its
            # operand/gate slices then get zero gradient
            if dy is None:
                sl(d_fused, xi).zero_()
                sl(d_fused, gi).zero_()
                return
            ext.gatemul_bwd(dy.contiguous(), sl(fused, xi), sl(fused, gi),
                            C5, C5, ctx.rm,
                            dx_out=sl(d_fused, xi), dg_out=sl(d_fused, gi),
                            dxs=C5, dgs=C5)

        bwd_pair(d_left, 0, 2)
        bwd_pair(d_right, 1, 3)
        if d_og is not None:
            sl(d_fused, 4).copy_(d_og)
        else:
            sl(d_fused, 4).zero_()
        return d_fused, None, None


def hip_tri_proj_gates(fused, hdim, rowmask=None):
    return _TriProjGatesFn.apply(fused, hdim, rowmask)


class _IPACoreFn(torch.autograd.Function):
    """Fused fp32 IPA attention core (K7): logits + masked softmax + the
    three value aggregations + local-frame transform in one kernel.
    When a gradient is required the forward also saves the
    probabilities (b,h,n,n) and the aggregated global points; the
    backward is a row-side plus a column-side kernel without atomics.
    dpair and drot are only computed when their inputs require grad."""

    @staticmethod
    @custom_fwd(device_type='cuda', cast_inputs=torch.float32)
    def forward(ctx, q_s, k_s, v_s, q_pg, k_pg, v_pg, bias, pair, rot,
                trans, point_w, mask, scales):
        ext = _load_ext()
        tensors = tuple(t.contiguous() for t in (
            q_s, k_s, v_s, q_pg, k_pg, v_pg, bias, pair, rot, trans,
            point_w))
        mask_c = mask.contiguous() if mask is not None else None
        save = any(ctx.needs_input_grad)
        out, attn, gpts = ext.ipa_core_fwd(*tensors, *scales, mask=mask_c,
                                           save_stats=save)
        if save:
            ctx.save_for_backward(attn, gpts, *tensors)
            ctx.mask = mask_c
            ctx.scales = scales
        return out

    @staticmethod
    @custom_bwd(device_type='cuda')
    @once_differentiable
    def backward(ctx, dout):
        ext = _load_ext()
        attn, gpts, *tensors = ctx.saved_tensors
        need = ctx.needs_input_grad
        grads = ext.ipa_core_bwd(dout.contiguous(), attn, gpts, *tensors,
                                 *ctx.scales, mask=ctx.mask,
                                 need_dpair=need[7], need_drot=need[8])
        return (*(g if n else None for g, n in zip(grads, need)),
                None, None)


def hip_ipa_core(q_s, k_s, v_s, q_pg, k_pg, v_pg, bias, pair, rot, trans,
                 point_w, scale_s, scale_b, scale_p, eps, mask=None):
    """q_s/k_s/v_s (b,n,h,16), q_pg/k_pg/v_pg (b,n,h,4,3) in the global
    frame, bias (b,h,n,n), pair (b,n,n,dp), rot (b,n,3,3), trans (b,n,3),
    point_w (h,) softplus-ed, mask (b,n) bool or None.  Returns the
    (b, n, h*(16 + dp + 16)) concatenation `to_out` consumes."""
    return _IPACoreFn.apply(q_s, k_s, v_s, q_pg, k_pg, v_pg, bias, pair,
                            rot, trans, point_w, mask,
                            (float(scale_s), float(scale_b), float(scale_p),
                             float(eps)))


def _dense16(t):
    """Contiguous and 16-byte aligned (the kernels read float4): a
    contiguous view at an odd offset of its storage is copied."""
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


class _SE3CoreFn(torch.autograd.Function):
    """Fused fp32 SE(3) refiner attention core (K15): qk + in-kernel pair
    bias Linear + distance term + key-masked softmax + value and
    displacement aggregation in one kernel.  When a gradient is required
    the forward also saves the probabilities (b,h,n,n); the backward is a
    row-side plus a column-side kernel without atomics.  dedges is only
    computed when `edges` requires grad."""

    @staticmethod
    @custom_fwd(device_type='cuda', cast_inputs=torch.float32)
    def forward(ctx, q, k, v, x, edges, w_e, b_e, mask, scale, eps,
                grad_enabled):
        ext = _load_ext()
        tensors = tuple(_dense16(t) for t in (q, k, v, x, edges, w_e, b_e))
        mask_c = mask.contiguous() if mask is not None else None
        # needs_input_grad mirrors requires_grad, also under no_grad, and
        # grad mode is always off in here: the caller passes the mode it
        # was called in, so that inference does not write A
        save = grad_enabled and any(ctx.needs_input_grad)
        out, dxh, attn = ext.se3_core_fwd(*tensors, scale, eps, mask=mask_c,
                                          save_attn=save)
        if save:
            ctx.save_for_backward(attn, *tensors)
            ctx.mask = mask_c
            ctx.scale, ctx.eps = scale, eps
        return out, dxh

    @staticmethod
    @custom_bwd(device_type='cuda')
    @once_differentiable
    def backward(ctx, dout, ddxh):
        ext = _load_ext()
        attn, *tensors = ctx.saved_tensors
        need = ctx.needs_input_grad
        grads = ext.se3_core_bwd(_dense16(dout), _dense16(ddxh), attn,
                                 *tensors, ctx.scale, ctx.eps, mask=ctx.mask,
                                 need_dedges=need[4])
        return (*(g if n else None for g, n in zip(grads, need)),
                None, None, None, None)


def hip_se3_core(q, k, v, x, edges, w_e, b_e, scale, eps, mask=None):
    """q/k/v (b,n,h*dh) as the Linears produce them, x (b,n,3), edges
    (b,n,n,e), w_e (h,e+1) / b_e (h,) the pair-bias Linear (last column
    of w_e multiplies |x_i - x_j|^2), mask (b,n) bool over keys or None.
    Returns (out (b,n,h*dh), dxh (b,n,h,3))."""
    return _SE3CoreFn.apply(q, k, v, x, edges, w_e, b_e, mask,
                            float(scale), float(eps),
                            torch.is_grad_enabled())


class _EGNNCoreFn(torch.autograd.Function):
    """Fused fp32 EGNN edge-message core (K16): first edge Linear on
    `edges` + distance term + the two 64x64 layers of edge_mlp / coors_mlp
    + both aggregations in one f32-MFMA kernel.  The forward writes
    nothing of pair size and saves its inputs only; the backward
    recomputes the chain in one kernel and stores dz1 (b,n,n,m), from
    which dedges and dW_e come as library GEMMs.  dedges is only computed
    when `edges` requires grad."""

    @staticmethod
    @custom_fwd(device_type='cuda', cast_inputs=torch.float32)
    def forward(ctx, P, Q, x, edges, W_e, w_d, W2, b2, Wc1, bc1, Wc2, bc2,
                mask, eps):
        ext = _load_ext()
        x = x.contiguous()                  # read as scalars: 4-byte aligned
        tensors = tuple(_dense16(t) for t in (
            P, Q, edges, W_e, w_d, W2, b2, Wc1, bc1, Wc2, bc2))
        P, Q, *rest = tensors
        tensors = (P, Q, x, *rest)
        mask_c = mask.contiguous() if mask is not None else None
        m_i, dx = ext.egnn_core_fwd(*tensors, eps, mask=mask_c)
        if any(ctx.needs_input_grad):
            ctx.save_for_backward(*tensors)
            ctx.mask = mask_c
            ctx.eps = eps
        return m_i, dx

    @staticmethod
    @custom_bwd(device_type='cuda')
    @once_differentiable
    def backward(ctx, dm, ddx):
        ext = _load_ext()
        tensors = ctx.saved_tensors
        edges, W_e = tensors[3], tensors[4]
        need = ctx.needs_input_grad
        (dP, dQ, dx, dz1, dw_d, dW2, db2, dWc1, dbc1, dWc2,
         dbc2) = ext.egnn_core_bwd(_dense16(dm), ddx.contiguous(), *tensors,
                                   ctx.eps, mask=ctx.mask)
        m = dz1.shape[-1]
        dz1 = dz1.view(-1, m)
        dedges = (dz1 @ W_e).view_as(edges) if need[3] else None
        dW_e = dz1.t() @ edges.view(-1, edges.shape[-1]) if need[4] else None
        grads = (dP, dQ, dx, dedges, dW_e, dw_d, dW2, db2, dWc1, dbc1, dWc2,
                 dbc2)
        return (*(g if n else None for g, n in zip(grads, need)),
                None, None)


def hip_egnn_core(P, Q, x, edges, W_e, w_d, W2, b2, Wc1, bc1, Wc2, bc2, eps,
                  mask=None):
    """P = W_i h + b1 and Q = W_j h (b,n,m), x (b,n,3), edges (b,n,n,e);
    W_e (m,e) / w_d (m,) the edge and distance columns of edge_mlp[0],
    W2/b2 = edge_mlp[2], Wc1/bc1 = coors_mlp[0], Wc2 (1,m) / bc2 (1,) =
    coors_mlp[2]; mask (b,n) bool or None.  Returns (m_i (b,n,m), the
    unclamped dx (b,n,3))."""
    return _EGNNCoreFn.apply(P, Q, x, edges, W_e, w_d, W2, b2, Wc1, bc1,
                             Wc2, bc2, mask, float(eps))


class _PairRepFn(torch.autograd.Function):
    """Fused pair-rep build (K13): out[b,i,j] = left[i] + right[j] +
    emb[rel[i,j]].  Forward writes the (b,n,n,d) tensor ONCE (the eager
    composition takes three full passes); backward is ext.pairrep_bwd: the
    three sums from one read of dy, no atomics."""

    @staticmethod
    @custom_fwd(device_type='cuda', cast_inputs=torch.bfloat16)
    def forward(ctx, left, right, emb, rel):
        ext = _load_ext()
        ctx.save_for_backward(rel)
        ctx.emb_rows = emb.shape[0]
        return ext.pairrep_fwd(left.contiguous(), right.contiguous(),
                               emb.contiguous(), rel.contiguous())

    @staticmethod
    @custom_bwd(device_type='cuda')
    def backward(ctx, dy):
        (rel,) = ctx.saved_tensors
        ext = _load_ext()
        if not _PAIRREP_BWD_V1 and ext.pairrep_bwd_covers(dy, ctx.emb_rows):
            dleft, dright, demb = ext.pairrep_bwd(dy, rel, ctx.emb_rows)
            return dleft, dright, demb, None
        return (*_pairrep_bwd_composed(dy, rel, ctx.emb_rows), None)


# AF2AMD_PAIRREP_BWD_V1=1 keeps the library composition below
_PAIRREP_BWD_V1 = _os.environ.get("AF2AMD_PAIRREP_BWD_V1", "0") == "1"


def _pairrep_bwd_composed(dy, rel, emb_rows):
    """Pair-rep backward from library ops: two wide sums and an fp32
    index_add (global float atomics, so demb is not reproducible).  The
    path of whatever ext.pairrep_bwd_covers turns down: a dy that is not
    contiguous, d above 1024 or no multiple of 8, a table beyond LDS."""
    d = dy.shape[-1]
    dleft = dy.sum(dim=2)
    dright = dy.sum(dim=1)
    demb = torch.zeros(emb_rows, d, device=dy.device, dtype=torch.float32)
    demb.index_add_(0, rel.reshape(-1), dy.reshape(-1, d).float())
    return dleft, dright, demb.to(dy.dtype)


def hip_pair_rep(left, right, emb, rel):
    return _PairRepFn.apply(left, right, emb, rel)


def _byte_mask(mask):
    """bool / uint8 mask as the contiguous one-byte tensor the kernels
    read; a contiguous bool mask is passed as it is (no copy)."""
    if mask is None:
        return None
    if mask.dtype not in (torch.bool, torch.uint8):
        mask = mask != 0
    return mask.contiguous()


class _TemplatePointwiseFn(torch.autograd.Function):
    """Template pointwise attention (K5): one query and T keys per pair
    position, q (b, P, H*d) and kv (b, T, P, 2*H*d) consumed in the
    layouts the projections produce (through their strides: nothing is
    permuted, padded or copied).  bf16 or fp32 storage, fp32 math.
    Forward keeps q, kv, out and lse (b, P, H); backward is one kernel
    writing dq and ONE dkv in kv's layout, so there is no split-backward
    concatenation.  The masks are not differentiable inputs and stay on
    ctx as the caller's own tensors."""

    @staticmethod
    @custom_fwd(device_type='cuda', cast_inputs=torch.bfloat16)
    def forward(ctx, q, kv, key_mask, query_mask, heads):
        ext = _load_ext()
        key_mask, query_mask = _byte_mask(key_mask), _byte_mask(query_mask)
        out, lse = ext.tplattn_fwd(q, kv, heads, key_mask=key_mask,
                                   query_mask=query_mask)
        ctx.save_for_backward(q, kv, out, lse)
        ctx.key_mask, ctx.query_mask = key_mask, query_mask
        ctx.heads = heads
        return out

    @staticmethod
    @custom_bwd(device_type='cuda')
    @once_differentiable
    def backward(ctx, dout):
        ext = _load_ext()
        q, kv, out, lse = ctx.saved_tensors
        dout = _dense16(dout.to(q.dtype))
        dq, dkv = ext.tplattn_bwd(dout, q, kv, out, lse, ctx.heads,
                                  key_mask=ctx.key_mask,
                                  query_mask=ctx.query_mask)
        return dq, dkv, None, None, None


def hip_template_pointwise(q, kv, heads, key_mask=None, query_mask=None):
    """q (b, P, H*d), kv (b, T, P, 2*H*d) = [k | v], key_mask (b, T, P)
    and query_mask (b, P) bool / uint8 or None.  Returns out (b, P, H*d).
    Operands need a dense last dim and 16-byte aligned rows; the launcher
    raises otherwise."""
    return _TemplatePointwiseFn.apply(q, kv, key_mask, query_mask,
                                      int(heads))
