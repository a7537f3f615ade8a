"""The decoder layer's arithmetic around attention, written once: what follows attention in the forward pass and
the two halves of the layer's backward.  Every formulation -- LlamaStack (functions.py) and the prefix-reuse episode's prefix, step,
lazy and batched walks (episode.py) -- drives these three functions; attention itself, the K/V cache traffic, RoPE and the step
tables differ between the formulations and stay with the callers.

Callers pass
  lw     the layer's operands (FlatStore.layer(i));
  dst    result name -> destination tensor; a missing name is allocated by the op (`out=None`);
  wgrad  (backward) what happens to a weight gradient: wgrad(name, dy, act, gout) with name in "down" | "gate_up" | "o" | "qkv" is
         called right after the dgrad GEMM that consumes the same dy.  `wgrad_now(epilogue)` runs the GEMM there, `wgrad_deferred`
         leaves it to the caller's one wide GEMM per weight;
  mark / before_write  (backward, optional) the hazard points of LlamaStack.backward's side-stream weight gradients: mark() before
         every dgrad GEMM that has a weight gradient riding along, before_write(name) before scratch result `name` is overwritten.
"""
from . import ops

_NO_DST = {}


def _nop(*_):
    return None


wgrad_deferred = _nop


def wgrad_now(epilogue):
    """the weight gradient as a GEMM of its own, at once: read-add (EPI_ACCUM) or first-writer store (EPI_STORE)"""
    def wgrad(name, dy, act, gout):
        ops.gemm_bf16(ops.TN, dy, act, out=gout, epilogue=epilogue)
    return wgrad


def bf16_linear(lw):
    """linear(a, kind, ...) = a W^T (+ R) on the layer's bf16 operands"""
    W = {"o": lw.Wo, "gate_up": lw.Wgu, "down": lw.Wd}

    def linear(a, kind, out=None, R=None, epilogue=ops.EPI_STORE):
        return ops.gemm_bf16(ops.NT, a, W[kind], out=out, R=R, epilogue=epilogue)
    return linear


def attn_out_mlp_fwd(lw, x, attn, eps, dst=_NO_DST, linear=None):
    """o_proj + residual -> RMSNorm -> gate|up -> SwiGLU -> down + residual on the rows of x (layer input) and attn (attention output).
    linear: NavModel.lm_linear bound to the layer where the weight-only fp8 deployment must stay reachable; default: the bf16 operands.
    -> x1, n2, rstd2, gu, h, x2"""
    out = dst.get
    linear = linear or bf16_linear(lw)
    x1 = linear(attn, "o", out=out("x1"), R=x, epilogue=ops.EPI_RESID)
    n2, rstd2 = ops.rmsnorm_fwd(x1, lw.w2, eps, out=out("n2"), rstd=out("rstd2"))
    gu = linear(n2, "gate_up", out=out("gu"))
    h = ops.swiglu_fwd(gu, out=out("h"))
    x2 = linear(h, "down", out=out("x2"), R=x1, epilogue=ops.EPI_RESID)
    return x1, n2, rstd2, gu, h, x2


def attn_out_mlp_bwd(lw, dx2, attn, x1, n2, rstd2, gu, h, dst=_NO_DST, wgrad=wgrad_deferred, mark=_nop, before_write=_nop, fuse_swiglu=False):
    """backward of attn_out_mlp_fwd from dx2 = d(x2): dgrad down, SwiGLU', dgrad gate|up, the post-attention norm's backward (+ dx2, the
    residual branch), dgrad o.  fuse_swiglu: SwiGLU' in the down-proj dgrad GEMM's epilogue (dh never reaches HBM).
    -> dx1, dattn, dgu"""
    out = dst.get
    if fuse_swiglu:
        before_write("dgu")
        dgu = ops.gemm_bf16(ops.NN, dx2, lw.Wd, out=out("dgu"), R=gu, epilogue=ops.EPI_SWIGLU_BWD)
        wgrad("down", dx2, h, lw.gd)
    else:
        mark()
        dh = ops.gemm_bf16(ops.NN, dx2, lw.Wd, out=out("dh"))
        wgrad("down", dx2, h, lw.gd)
        before_write("dgu")
        dgu = ops.swiglu_bwd(gu, dh, out=out("dgu"))
    mark()
    dn2 = ops.gemm_bf16(ops.NN, dgu, lw.Wgu, out=out("dn2"))
    wgrad("gate_up", dgu, n2, lw.ggu)
    before_write("dx1")
    dx1 = ops.rmsnorm_bwd(dn2, x1, lw.w2, rstd2, lw.gw2, resid_grad=dx2, out=out("dx1"))
    mark()
    dattn = ops.gemm_bf16(ops.NN, dx1, lw.Wo, out=out("dattn"))
    wgrad("o", dx1, attn, lw.go)
    return dx1, dattn, dgu


def qkv_in_bwd(lw, dqkv, x, n1, rstd1, resid, dst=_NO_DST, wgrad=wgrad_deferred, mark=_nop, before_write=_nop):
    """backward of the layer's head from dqkv (pre-RoPE frame): dgrad q|k|v, the input norm's backward (+ resid = dx1, the residual
    branch; None: no residual gradient).  -> dx, the gradient of the layer input"""
    out = dst.get
    mark()
    dn1 = ops.gemm_bf16(ops.NN, dqkv, lw.Wqkv, out=out("dn1"))
    wgrad("qkv", dqkv, n1, lw.gqkv)
    before_write("dx")
    return ops.rmsnorm_bwd(dn1, x, lw.w1, rstd1, lw.gw1, resid_grad=resid, out=out("dx"))
