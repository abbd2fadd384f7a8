"""Backend dispatch between the gfx950 HIP extension and the eager path.

Policy:
* CPU tensors -> eager, always.
* ROCm tensors + extension loaded -> HIP kernel when one exists for the
  op (per-op hasattr check so kernels can land incrementally), else the
  eager composition (which still runs on-device through rocBLAS/hipBLASLt).
* ROCm tensors + extension NOT importable -> hard error ("native code not
  loaded") unless AF2AMD_ALLOW_EAGER_GPU=1.
* AF2AMD_FORCE_EAGER=1 pins eager everywhere (kernel parity tests).
"""
import os

import torch

from . import eager

_FORCE_EAGER = os.environ.get("AF2AMD_FORCE_EAGER", "0") == "1"
_ALLOW_EAGER_GPU = os.environ.get("AF2AMD_ALLOW_EAGER_GPU", "0") == "1"

_EXT = None
_EXT_TRIED = False
_EXT_ERR = None


def _load_ext():
    global _EXT, _EXT_TRIED, _EXT_ERR
    if _EXT_TRIED:
        return _EXT
    _EXT_TRIED = True
    try:
        from alphafold2_amd import _hip_ops  # built in-tree for gfx950
        _EXT = _hip_ops
    except ImportError as e:  # extension not built (CPU-only dev box)
        _EXT = None
        _EXT_ERR = e
    return _EXT


def hip_ops_available():
    return _load_ext() is not None


def _want_hip(t: torch.Tensor) -> bool:
    if _FORCE_EAGER or not t.is_cuda:
        return False
    ext = _load_ext()
    if ext is None:
        if _ALLOW_EAGER_GPU:
            return False
        raise RuntimeError(
            "alphafold2_amd._hip_ops is not importable on a GPU device "
            f"(build with `python setup.py build_ext --inplace`): {_EXT_ERR}")
    return True


def using_hip(t: torch.Tensor, opname: str) -> bool:
    """True when `opname` should run through the HIP extension."""
    return _want_hip(t) and hasattr(_load_ext(), opname)


_warned = set()


def warn_gpu_fallback(opname: str, reason: str):
    """Log (once per op+reason) when a GPU tensor takes the eager path
    even though the extension is loaded — silent fallbacks hide
    'MI355X-native in name only' configs."""
    key = (opname, reason)
    if key in _warned or _FORCE_EAGER:
        return
    _warned.add(key)
    import warnings
    warnings.warn(
        f"alphafold2_amd: op '{opname}' is running the EAGER composition "
        f"on GPU ({reason}); the fused gfx950 kernel does not cover this "
        "configuration", RuntimeWarning, stacklevel=3)


# ---------------------------------------------------------------------------
# op entry points


def _attn_unfusable_reason(t, dim_head, bias, drop_p, tie_dim=None,
                           batch=None, dtype=None):
    """None when the fused attention kernels cover the configuration,
    else the text naming the predicate that failed.  `t` is the bf16
    q (or packed) tensor (`dtype` overrides its dtype when the tensor the
    kernels will see does not exist yet); drop_p the ACTIVE dropout rate
    (0 when off).  A missing extension is not judged here (`_want_hip`
    raises or allows eager for it)."""
    ext = _load_ext()
    if dtype is None:
        dtype = t.dtype
    if ext is not None and not hasattr(ext, 'attn_fwd'):
        return 'extension built without attn_fwd'
    if (ext is not None and drop_p > 0.
            and not hasattr(ext, 'attn_dropout_mask')):
        return ('attention-prob dropout active and the extension was built '
                'without attn_dropout_mask')
    if drop_p >= 1.:
        return f'attention-prob dropout p={drop_p} (fused kernel needs p < 1)'
    if not (dim_head <= 64 and dim_head % 8 == 0):
        return (f'dim_head={dim_head} (fused kernel covers '
                'multiples of 8 up to 64)')
    if dtype != torch.bfloat16:
        return f'dtype={dtype} (fused kernel is bf16)'
    if bias is not None and bias.dtype != torch.bfloat16:
        return f'bias dtype={bias.dtype} (fused kernel is bf16)'
    if tie_dim is not None and batch % tie_dim != 0:
        return f'batch {batch} is not divisible by tie_dim={tie_dim}'
    return None


def attention_core(q, k, v, bias=None, mask=None, context_mask=None,
                   tie_dim=None, bias_repeat=1, dropout=0., training=False):
    """bias (when given) has shape (B // bias_repeat, h, Lq, Lk); the
    repeat fold is resolved inside the fused kernel (never materialized),
    and expanded explicitly only on the eager path.  Attention-prob
    dropout (reference alphafold2.py:172) runs inside the fused kernels
    when `dropout > 0 and training`."""
    drop_p = float(dropout) if (dropout > 0. and training) else 0.
    # head dims < 64 run on the 64-wide tile via zero padding (see
    # hip_attention_core); only dim_head > 64 or non-multiple-of-8
    # layouts fall back to eager
    if q.is_cuda and not _FORCE_EAGER:
        reason = _attn_unfusable_reason(q, q.shape[-1], bias, drop_p,
                                        tie_dim, q.shape[0])
        if reason is not None:
            if hip_ops_available():
                warn_gpu_fallback('attention_core', reason)
        elif _want_hip(q):
            from .hip_autograd import hip_attention_core
            return hip_attention_core(q, k, v, bias=bias, mask=mask,
                                      context_mask=context_mask,
                                      tie_dim=tie_dim,
                                      bias_repeat=bias_repeat,
                                      dropout_p=drop_p)
    if bias is not None and bias_repeat != 1:
        bias = bias.repeat_interleave(bias_repeat, dim=0)
    return eager.attention_core(q, k, v, bias=bias, mask=mask,
                                context_mask=context_mask, tie_dim=tie_dim,
                                dropout=dropout, training=training)


# AF2AMD_GATED_ATTN_UNIT=0 keeps gated self-attention on the separate
# projection / packed attention / gate Functions (A/B measurement)
_GATED_ATTN_UNIT = os.environ.get("AF2AMD_GATED_ATTN_UNIT", "1") != "0"


def _gated_unit_ok(x, w_cat, gate_bias, heads, inner, bias, drop_p):
    """True when hip_autograd._GatedAttentionUnitFn covers gated
    self-attention from its input x (B, L, d): switch on, HIP in use,
    head dim 64, bf16 operands (or fp32 under bf16 autocast) and whatever
    the fused attention kernels themselves ask for."""
    return (
        _GATED_ATTN_UNIT
        and x.is_cuda and x.dim() == 3
        and w_cat.shape[0] == 4 * inner
        and inner == heads * 64
        and _bf16_ok(x, w_cat, gate_bias)
        and _attn_unfusable_reason(x, 64, bias, drop_p,
                                   dtype=torch.bfloat16) is None
        and using_hip(x, 'attn_gate_bwd')
    )


def attention_core_packed(packed, heads, inner, bias=None, mask=None,
                          context_mask=None, bias_repeat=1, dropout=0.,
                          training=False, gated_input=None):
    """Self-attention consuming a packed [q|k|v|...] projection (B, L, W).
    HIP-only fast path; returns None if not fusable (caller falls back
    to the split path, whose dispatch names the reason).

    gated_input=(x, w_cat, gate_bias), with packed=None, asks for gated
    self-attention as ONE autograd unit from the block input x (B, L, d):
    projection by w_cat = [to_q | to_kv | gating] weights (4 * inner, d),
    attention core and sigmoid output gate.  Returns the gated
    (B, L, inner) output, or None when the unit does not cover the
    configuration (the caller then projects and calls again without
    gated_input)."""
    key_mask = context_mask if context_mask is not None else mask
    drop_p = float(dropout) if (dropout > 0. and training) else 0.
    if gated_input is not None:
        x, w_cat, gate_bias = gated_input
        if not _gated_unit_ok(x, w_cat, gate_bias, heads, inner, bias,
                              drop_p):
            return None
        from .hip_autograd import hip_attention_packed
        return hip_attention_packed(None, heads, inner, bias=bias,
                                    mask=key_mask, bias_repeat=bias_repeat,
                                    dropout_p=drop_p,
                                    gated_input=gated_input)
    fusable = (
        packed.is_cuda
        and (inner // heads) == 64
        and _attn_unfusable_reason(packed, 64, bias, drop_p) is None
        and _want_hip(packed)
    )
    if not fusable:
        return None
    from .hip_autograd import hip_attention_packed
    return hip_attention_packed(packed, heads, inner, bias=bias,
                                mask=key_mask, bias_repeat=bias_repeat,
                                dropout_p=drop_p)


def geglu(x):
    if using_hip(x, 'geglu_fwd'):
        from .hip_autograd import hip_geglu
        return hip_geglu(x)
    return eager.geglu(x)


def _bf16_ok(*tensors):
    """True when every tensor is bf16 already, or will be autocast to
    bf16 inside the custom_fwd wrapper (fp32 under cuda bf16 autocast)."""
    amp = (torch.is_autocast_enabled('cuda')
           and torch.get_autocast_dtype('cuda') == torch.bfloat16)
    for t in tensors:
        if t is None:
            continue
        if t.dtype == torch.bfloat16:
            continue
        if amp and t.dtype in (torch.float32, torch.float16):
            continue
        return False
    return True


def fused_linear(x, weight, bias=None, residual=None):
    """out = x @ weight.T (+ bias) (+ residual).

    Measured (profiles/r02_ffgemm_ab.log): hipBLASLt beats the custom
    128x128 GEMM on plain/residual FORWARDS, so _LinearFn runs Tensile
    forward by default (AF2AMD_CUSTOM_LINEAR=1 forces the custom GEMM
    for A/B work); the routing still pays in backward, where the
    streaming split-K wgrad kernel takes the huge-K weight gradient and
    returns the bias gradient from the same pass."""
    ok = (x.shape[-1] % 8 == 0 and weight.shape[0] % 8 == 0
          and _bf16_ok(x, weight, residual)
          and using_hip(x, 'linear_fwd'))
    if ok:
        from .hip_autograd import hip_linear
        return hip_linear(x, weight, bias, residual)
    out = torch.nn.functional.linear(x, weight, bias)
    if residual is not None:
        out = out + residual
    return out


def ff1_geglu(x, weight, bias=None):
    """GEGLU(x @ weight.T + bias) with the GEMM + chunk + gelu + mul
    fused into one kernel (K6 of SURVEY.md §2.17)."""
    ok = (x.shape[-1] % 8 == 0 and weight.shape[0] % 16 == 0
          and _bf16_ok(x, weight)
          and using_hip(x, 'ff1_geglu_fwd'))
    if ok:
        if not torch.is_grad_enabled():
            # inference: skip materializing the 2x-width pre-activation
            ext = _load_ext()
            x16, w16, b16 = (t.to(torch.bfloat16).contiguous()
                             if t is not None else None
                             for t in (x, weight, bias))
            return ext.ff1_geglu_fwd(x16, w16, b16, -1, False)[0]
        from .hip_autograd import hip_ff1_geglu
        return hip_ff1_geglu(x, weight, bias)
    return geglu(torch.nn.functional.linear(x, weight, bias))


def outer_product_mean(left, right, mask=None, eps=1e-5):
    if left.dtype == torch.bfloat16 and using_hip(left, 'pcgemm'):
        from .hip_autograd import hip_outer_product_mean
        return hip_outer_product_mean(left, right, mask=mask, eps=eps)
    return eager.outer_product_mean(left, right, mask=mask, eps=eps)


def triangle_mix(left, right, mix):
    if left.dtype == torch.bfloat16 and using_hip(left, 'pcgemm'):
        from .hip_autograd import hip_triangle_mix
        return hip_triangle_mix(left, right, mix)
    return eager.triangle_mix(left, right, mix)


def pair_outer_sum(x_left, x_right):
    return eager.pair_outer_sum(x_left, x_right)


def pair_rep_build(x_left, x_right, emb_weight, rel):
    """K13: out[b,i,j] = left[i] + right[j] + emb[rel[i,j]] in one pass
    (the eager composition materializes the outer sum AND the gathered
    embedding before adding)."""
    ok = (x_left.shape[-1] % 8 == 0 and x_left.shape[-1] <= 2048
          and _bf16_ok(x_left, x_right, emb_weight)
          and using_hip(x_left, 'pairrep_fwd'))
    if ok:
        from .hip_autograd import hip_pair_rep
        rel = rel.expand(x_left.shape[0], -1, -1).contiguous().long()
        return hip_pair_rep(x_left, x_right, emb_weight, rel)
    return eager.pair_outer_sum(x_left, x_right) \
        + torch.nn.functional.embedding(rel, emb_weight)


def distance_buckets(coords, boundaries):
    if using_hip(coords, 'dist_buckets'):
        ext = _load_ext()
        return ext.dist_buckets(coords.contiguous(), boundaries.contiguous())
    return eager.distance_buckets(coords, boundaries)


def ipa_core_fusable(x, pairwise_repr, *, heads, scalar_key_dim,
                     scalar_value_dim, point_key_dim, point_value_dim,
                     require_pairwise_repr):
    """Gate of the fused IPA core (K7, forward and backward).  True when
    `hip_autograd.hip_ipa_core` covers the configuration; otherwise the
    caller runs the eager composition and, on a GPU with the extension
    loaded, the failed predicate is named in a fallback warning.  Looks
    at shapes and host-side device properties only: no device sync, so
    the gate is safe inside hipGraph capture."""
    if not _want_hip(x):
        return False
    ext = _load_ext()
    n = x.shape[1]
    pair_dim = pairwise_repr.shape[-1] if pairwise_repr is not None else 0
    if not hasattr(ext, 'ipa_core_bwd'):
        reason = 'extension built without ipa_core_bwd'
    elif not require_pairwise_repr or pairwise_repr is None:
        reason = 'require_pairwise_repr=False'
    elif not 1 <= heads <= 8:
        reason = f'heads={heads} (fused kernel covers 1 to 8)'
    elif (scalar_key_dim, scalar_value_dim) != (16, 16):
        reason = (f'scalar dims {scalar_key_dim}/{scalar_value_dim} '
                  '(fused kernel covers 16/16)')
    elif (point_key_dim, point_value_dim) != (4, 4):
        reason = (f'point dims {point_key_dim}/{point_value_dim} '
                  '(fused kernel covers 4/4)')
    elif pair_dim % 64 != 0 or not 64 <= pair_dim <= 512:
        reason = (f'pair dim {pair_dim} (fused kernel covers multiples '
                  'of 64 up to 512)')
    elif x.dtype == torch.float64:
        reason = 'dtype=torch.float64 (fused kernel is fp32)'
    elif n > ext.ipa_core_max_n(heads, pair_dim):
        reason = (f'n={n} exceeds the LDS bound '
                  f'{ext.ipa_core_max_n(heads, pair_dim)} for heads={heads}')
    else:
        return True
    warn_gpu_fallback('ipa_core', reason)
    return False


def _se3_fused_enabled():
    # read per call so an A/B measurement can flip it inside one process
    return os.environ.get("AF2AMD_SE3_FUSED", "1") != "0"


def se3_core_fusable(h, edges, *, heads, dim_head):
    """Gate of the fused SE(3) refiner attention core (K15, forward and
    backward).  True when `hip_autograd.hip_se3_core` covers the
    configuration; otherwise the caller runs the eager composition and,
    on a GPU with the extension loaded, the failed predicate is named in
    a fallback warning.  AF2AMD_SE3_FUSED=0 turns the fused path off
    without a warning (A/B measurement).  Looks at shapes and host-side
    properties only: no device sync, so the gate is safe inside hipGraph
    capture.  It must not look at the capture state either: a step whose
    warmup ran the fused core and whose capture ran the eager
    composition would issue that composition's GEMMs for the first time
    under capture, which hipBLASLt refuses ('operation not permitted
    when stream is capturing') and which ends the process."""
    if not _se3_fused_enabled() or not _want_hip(h):
        return False
    ext = _load_ext()
    n = h.shape[1]
    edge_dim = edges.shape[-1] if edges is not None else 0
    autocast = torch.is_autocast_enabled('cuda')
    if not hasattr(ext, 'se3_core_bwd'):
        reason = 'extension built without se3_core_bwd'
    elif edges is None:
        reason = 'edges=None'
    elif not 1 <= heads <= 8:
        reason = f'heads={heads} (fused kernel covers 1 to 8)'
    elif dim_head % 4 != 0 or not 4 <= dim_head <= 64:
        reason = (f'dim_head={dim_head} (fused kernel covers multiples '
                  'of 4 up to 64)')
    elif edge_dim % 64 != 0 or not 64 <= edge_dim <= 512:
        reason = (f'edge dim {edge_dim} (fused kernel covers multiples '
                  'of 64 up to 512)')
    elif h.dtype == torch.float64:
        reason = 'dtype=torch.float64 (fused kernel is fp32)'
    elif not autocast and (h.dtype != torch.float32
                           or edges.dtype != torch.float32):
        # under autocast custom_fwd casts every operand to fp32
        reason = (f'dtype={h.dtype} / edges {edges.dtype} outside autocast '
                  '(fused kernel is fp32)')
    elif n > ext.se3_core_max_n(heads, dim_head, edge_dim):
        reason = (f'n={n} exceeds the LDS bound '
                  f'{ext.se3_core_max_n(heads, dim_head, edge_dim)} for '
                  f'heads={heads}')
    else:
        return True
    warn_gpu_fallback('se3_core', reason)
    return False


def _egnn_fused_enabled():
    # read per call so an A/B measurement can flip it inside one process
    return os.environ.get("AF2AMD_EGNN_FUSED", "1") != "0"


def egnn_core_fusable(h, edges, *, m_dim):
    """Gate of the fused EGNN edge-message core (K16, forward and
    backward).  Same contract as `se3_core_fusable`: True when
    `hip_autograd.hip_egnn_core` covers the configuration; otherwise the
    caller runs the eager composition and, on a GPU with the extension
    loaded, the failed predicate is named in a fallback warning.
    AF2AMD_EGNN_FUSED=0 turns the fused path off without a warning (A/B
    measurement).  Shapes and host-side properties only: no device sync
    and no look at the capture state.  The kernels tile the keys, so
    there is no bound on n; the edge dim is bounded by the LDS copy of
    its weight."""
    if not _egnn_fused_enabled() or not _want_hip(h):
        return False
    ext = _load_ext()
    edge_dim = edges.shape[-1] if edges is not None else 0
    autocast = torch.is_autocast_enabled('cuda')
    if not hasattr(ext, 'egnn_core_bwd'):
        reason = 'extension built without egnn_core_bwd'
    elif edges is None:
        reason = 'edges=None'
    elif m_dim != 64:
        reason = f'm_dim={m_dim} (fused kernel covers 64)'
    elif edge_dim % 64 != 0 or not 64 <= edge_dim <= 512:
        reason = (f'edge dim {edge_dim} (fused kernel covers multiples '
                  'of 64 up to 256)')
    elif edge_dim > ext.egnn_core_max_edge_dim():
        reason = (f'edge dim {edge_dim} exceeds '
                  f'{ext.egnn_core_max_edge_dim()}, the widest first-layer '
                  'weight the kernels stage in LDS (320 to 512 need '
                  'K-chunked staging)')
    elif h.dtype == torch.float64:
        reason = 'dtype=torch.float64 (fused kernel is fp32)'
    elif not autocast and (h.dtype != torch.float32
                           or edges.dtype != torch.float32):
        # under autocast custom_fwd casts every operand to fp32
        reason = (f'dtype={h.dtype} / edges {edges.dtype} outside autocast '
                  '(fused kernel is fp32)')
    else:
        return True
    warn_gpu_fallback('egnn_core', reason)
    return False


def _template_pool_fused_enabled():
    # read per call so an A/B measurement can flip it inside one process
    return os.environ.get("AF2AMD_TEMPLATE_POOL_FUSED", "1") != "0"


# Largest template count the pointwise kernels (K5) are routed to.  It
# covers constants.MAX_NUM_TEMPLATES (10) with room to spare; it is NOT a
# measured crossover against the flash tile kernel, whose 64-row K/V tile
# only starts to fill at several times this count (no T-crossover study
# has been run; the kernels themselves loop over any T).
TEMPLATE_POOL_MAX_TEMPLATES = 16
_TEMPLATE_POOL_HEAD_DIMS = (8, 16, 32, 64)


def template_pool_fusable(q, kv, *, heads, dim_head, num_templates, drop_p):
    """Gate of the template pointwise attention kernels (K5, forward and
    backward).  True when `hip_autograd.hip_template_pointwise` covers the
    configuration.  Otherwise the caller takes the folded route through
    `attention_core`, which is the flash kernels wherever they apply; a
    fallback warning names the failed predicate only where that route
    would itself end in the eager composition.
    AF2AMD_TEMPLATE_POOL_FUSED=0 turns the path off without a warning (A/B
    measurement).  Same contract as `se3_core_fusable`: shapes and
    host-side properties only, no device sync and no look at the capture
    state.  q and kv may be the projections' inputs instead of their
    outputs: only device and dtype are read from them, and a Linear keeps
    both."""
    if not _template_pool_fused_enabled() or not _want_hip(q):
        return False
    ext = _load_ext()
    fp32_pair = q.dtype == torch.float32 and kv.dtype == torch.float32
    if not hasattr(ext, 'tplattn_bwd'):
        reason = 'extension built without tplattn_bwd'
    elif dim_head not in _TEMPLATE_POOL_HEAD_DIMS:
        # the d / 8 lanes of a (position, head) group must be a power of two
        reason = (f'dim_head={dim_head} (pointwise kernel covers '
                  '8, 16, 32 and 64)')
    elif heads < 1:
        reason = f'heads={heads}'
    elif not 1 <= num_templates <= TEMPLATE_POOL_MAX_TEMPLATES:
        reason = (f'{num_templates} templates (pointwise kernel is routed '
                  f'up to {TEMPLATE_POOL_MAX_TEMPLATES})')
    elif not (fp32_pair or _bf16_ok(q, kv)):
        reason = (f'dtype={q.dtype} / kv {kv.dtype} (pointwise kernel is '
                  'bf16 or fp32)')
    elif drop_p > 0.:
        reason = (f'attention-prob dropout p={drop_p} active (not in the '
                  'pointwise kernel)')
    else:
        return True
    # today's route is fused too: speak up only where it is not
    amp = (torch.is_autocast_enabled('cuda')
           and torch.get_autocast_dtype('cuda') == torch.bfloat16)
    flash_dtype = torch.bfloat16 if amp and q.is_floating_point() else q.dtype
    if _attn_unfusable_reason(q, dim_head, None, drop_p,
                              dtype=flash_dtype) is not None:
        warn_gpu_fallback('template_pool', reason)
    return False


def template_pointwise_attention(q, kv, heads, key_mask=None,
                                 query_mask=None):
    """Attention of ONE query per position over T keys (template pooling).

    * q:  (b, P, H*d), the query projection
    * kv: (b, T, P, 2*H*d), the [k | v] projection of the T contexts;
      head h owns channels [h*d, (h+1)*d) of each half
    * key_mask (b, T, P) / query_mask (b, P): bool, independent, optional
    Returns (b, P, H*d).  A logit whose key or query is masked is filled
    with -max before the softmax, so a position with every logit masked
    averages v over T.  The key mask is applied whether or not a query
    mask comes with it (eager.attention_core alone applies it only with
    one, so an all-true query mask is passed along there).

    On gfx950 this is `hip_template_pointwise`; on CPU, or where
    `template_pool_fusable` declines, the operands are folded to
    (b*P, H, 1|T, d) for `attention_core`."""
    b, P, C = q.shape
    T = kv.shape[1]
    d = C // heads
    if q.is_cuda and template_pool_fusable(
            q, kv, heads=heads, dim_head=d, num_templates=T, drop_p=0.):
        from .hip_autograd import hip_template_pointwise
        return hip_template_pointwise(q, kv, heads, key_mask=key_mask,
                                      query_mask=query_mask)
    qf = q.reshape(b * P, 1, heads, d).transpose(1, 2)
    k, v = (t.permute(0, 2, 1, 3).reshape(b * P, T, heads, d).transpose(1, 2)
            for t in kv.chunk(2, dim=-1))
    km = qm = None
    if key_mask is not None:
        km = key_mask.permute(0, 2, 1).reshape(b * P, T).bool()
    if query_mask is not None:
        qm = query_mask.reshape(b * P, 1).bool()
    if km is not None and qm is None:
        qm = torch.ones(b * P, 1, dtype=torch.bool, device=q.device)
    if qm is not None and km is None:
        km = torch.ones(1, T, dtype=torch.bool, device=q.device)
    out = attention_core(qf, k, v, mask=qm, context_mask=km)
    return out.transpose(1, 2).reshape(b, P, C)


def layer_norm(x, weight, bias, eps=1e-5):
    if using_hip(x, 'layernorm_fwd'):
        from .hip_autograd import hip_layer_norm
        return hip_layer_norm(x, weight, bias, eps)
    return eager.layer_norm(x, weight, bias, eps)


def tri_proj_gates(fused, hdim, row_mask=None):
    """TriangleMultiplicative's [left|right|lg|rg|og] projection -> the
    two gated operands + the out-gate slice, as ONE autograd unit whose
    backward writes into a packed buffer (kills the 5-way SplitBackward
    concatenation)."""
    ok = (fused.dtype == torch.bfloat16 and fused.shape[-1] == 5 * hdim
          and hdim % 8 == 0 and using_hip(fused, 'gatemul_bwd'))
    if ok:
        from .hip_autograd import hip_tri_proj_gates
        return hip_tri_proj_gates(fused, hdim, row_mask)
    left, right, lg, rg, og = fused.split([hdim] * 5, dim=-1)
    left = eager.softclamp_gate(left, lg)
    right = eager.softclamp_gate(right, rg)
    if row_mask is not None:
        m = row_mask.unsqueeze(-1).to(left.dtype)
        left = left * m
        right = right * m
    return left, right, og


def softclamp_gate(x, gates, row_mask=None):
    """out = x * sigmoid(gates) (* row_mask broadcast per row).
    row_mask: optional bool with shape == x.shape[:-1]."""
    # the kernel reads both operands as x's dtype: a mixed pair (e.g. an
    # fp32 residual with bf16 gates) takes the eager composition
    if (x.shape == gates.shape and x.dtype == gates.dtype
            and using_hip(x, 'gatemul_fwd')):
        from .hip_autograd import hip_gatemul
        return hip_gatemul(x, gates, row_mask)
    out = eager.softclamp_gate(x, gates)
    if row_mask is not None:
        out = out * row_mask.unsqueeze(-1).to(out.dtype)
    return out
