"""Adapter-v2 fine-tuning on an MI355X (csrc/adapter_v2.hip, include/fastmax_hip_adapter.h, fastmax_experiments_amd/adapter_v2.py).

y and dz are compared bit for bit with the tensor-op form on the device and with the explicit-rounding restatement of
adapter_v2_ref.py; dscale and dbias against the float64 sums of the same terms within the allowance derived there,
(M + 2) 2^-24 sum|term|.  Shapes: the smallest at which the kernels can go wrong -- a scalar row (N = 1, 7), a whole-piece row
(24), a row wider than one workgroup's slab of 64 pieces (2056); row counts around the edges of the row block R and of the
last-stage sum, which splits the blocks over four waves (1, 3, 4, 5 and 10 blocks)."""
import copy

import pytest
import torch

import adapter_v2_ref as ar
from conftest import golden_names, load_golden

pytestmark = pytest.mark.gpu

TD = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
PAIRS = [("f32", "f32"), ("bf16", "bf16"), ("f16", "f16"), ("bf16", "f32"), ("f16", "f32")]
CASES = [n for n in golden_names("adapterv2_") if n != "adapterv2_filter"]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from fastmax_experiments_amd import _lib
    _lib.lib()          # fail loudly if the extension is missing


def _rand(shape, seed, dt, scale=1.0, shift=0.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale + shift).to(dt).cuda()


def _operands(M, N, dt, pdt, seed):
    """z, scale (one column exactly 0 when there is more than one), bias, dy"""
    z = _rand((M, N), seed, TD[dt], 1.5)
    scale = _rand((N,), seed + 1, torch.float32, 0.5, 1.0)
    bias = _rand((N,), seed + 2, torch.float32, 0.5)
    if pdt != dt:                              # float32 values that no 16-bit number holds
        scale, bias = scale * (1.0 + 2.0 ** -12), bias + 2.0 ** -13
    if N > 1:
        scale[N // 3] = 0.0
    scale, bias = scale.to(TD[pdt]), bias.to(TD[pdt])
    dy = _rand((M, N), seed + 3, torch.promote_types(TD[dt], TD[pdt]))
    return z, scale, bias, dy


def _check(z, scale, bias, dy, what):
    """forward and backward through the kernels against both restatements; -> (y, dz, dscale, dbias)"""
    from fastmax_experiments_amd import adapter_v2 as av2
    y = av2.adapter_forward(z, scale, bias)
    dz, dsc, dbi = av2.adapter_backward(dy, z, scale, bias)
    r = ar.restate(z, scale, bias, dy)
    ty, tdz, _, _ = ar.tensor_op(z, scale, bias, dy)
    assert y.dtype == ty.dtype == r["y"].dtype and y.shape == z.shape
    assert torch.equal(y, ty) and torch.equal(y, r["y"]), what
    assert dz.dtype == z.dtype and torch.equal(dz, tdz) and torch.equal(dz, r["dz"]), what
    assert dsc.dtype == dbi.dtype == torch.float32 and dsc.shape == dbi.shape == scale.shape
    print(f"{what}: dscale {ar.worst(dsc, r['dscale64'], r['allow_scale']):.3f}, dbias {ar.worst(dbi, r['dbias64'], r['allow_bias']):.3f} "
          "of the allowance")
    assert ar.within(dsc, r["dscale64"], r["allow_scale"]), what
    assert ar.within(dbi, r["dbias64"], r["allow_bias"]), what
    return y, dz, dsc, dbi


# ---- 1. the kernels ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 7, 24, 2056])
@pytest.mark.parametrize("dt,pdt", PAIRS)
def test_kernels_against_the_restatements(dt, pdt, N):
    from fastmax_experiments_amd import adapter_v2 as av2
    R = av2.ROWS_PER_BLOCK
    for i, M in enumerate((1, R - 1, R, R + 1, 3 * R, 4 * R, 4 * R + 3, 9 * R + 1)):
        z, scale, bias, dy = _operands(M, N, dt, pdt, 1000 + 10 * i)
        _, _, dsc, dbi = _check(z, scale, bias, dy, f"{dt}/{pdt} M={M} N={N}")
        if N > 1:                               # a zero scale: no gradient reaches z there, the scale's own gradient is whole
            assert float(dbi[N // 3]) == 0.0 and float(dsc[N // 3].abs()) > 0.0
        again = av2.adapter_backward(dy, z, scale, bias)
        assert torch.equal(again[1], dsc) and torch.equal(again[2], dbi)          # a second call: the same bits


@pytest.mark.parametrize("dt,pdt", PAIRS)
def test_row_strides_a_misaligned_base_and_absent_outputs(dt, pdt):
    from fastmax_experiments_amd import adapter_v2 as av2
    M, N = av2.ROWS_PER_BLOCK + 5, 24
    z, scale, bias, dy = _operands(M, N, dt, pdt, 2000)
    want = _check(z, scale, bias, dy, f"{dt}/{pdt} contiguous")
    # a column slice of a wider buffer: the row stride is larger than N, rows still whole 16-byte pieces
    wide_z, wide_dy = torch.zeros((M, N + 16), dtype=z.dtype, device="cuda"), torch.zeros((M, N + 40), dtype=dy.dtype, device="cuda")
    wide_z[:, 8:8 + N], wide_dy[:, 32:32 + N] = z, dy
    zs, dys = wide_z[:, 8:8 + N], wide_dy[:, 32:32 + N]
    assert zs.stride(0) == N + 16 and not zs.is_contiguous()
    got = _check(zs, scale, bias, dys, f"{dt}/{pdt} row stride")
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    # a base one element off a 16-byte piece: the scalar path, the same bits
    flat_z, flat_dy = torch.zeros(M * N + 1, dtype=z.dtype, device="cuda"), torch.zeros(M * N + 1, dtype=dy.dtype, device="cuda")
    zo, dyo = flat_z[1:].view(M, N), flat_dy[1:].view(M, N)
    zo.copy_(z), dyo.copy_(dy)
    assert zo.data_ptr() % 16 != 0 and dyo.data_ptr() % 16 != 0
    got = _check(zo, scale, bias, dyo, f"{dt}/{pdt} misaligned")
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    # misaligned parameters alone do the same
    so, bo = (torch.cat([p[:1], p])[1:] for p in (scale, bias))
    assert so.data_ptr() % 16 != 0
    got = _check(z, so, bo, dy, f"{dt}/{pdt} misaligned parameters")
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    # dz absent, the sums absent
    only_sums = av2.adapter_backward(dy, z, scale, bias, want_dz=False)
    assert only_sums[0] is None and torch.equal(only_sums[1], want[2]) and torch.equal(only_sums[2], want[3])
    only_dz = av2.adapter_backward(dy, z, scale, bias, want_param_grads=False)
    assert only_dz[1] is None and only_dz[2] is None and torch.equal(only_dz[0], want[1])
    assert av2.adapter_backward(dy, z, scale, bias, want_dz=False, want_param_grads=False) == (None, None, None)
    # leading dimensions and no rows at all
    y3 = av2.adapter_forward(z.view(1, M, N), scale, bias)
    assert y3.shape == (1, M, N) and torch.equal(y3[0], want[0])
    empty = av2.adapter_forward(z[:0], scale, bias)
    assert empty.shape == (0, N) and empty.dtype == want[0].dtype
    e = av2.adapter_backward(dy[:0], z[:0], scale, bias)
    assert e[0].shape == (0, N) and float(e[1].abs().sum()) == 0.0 and float(e[2].abs().sum()) == 0.0


@pytest.mark.parametrize("name", CASES)
def test_fixtures_through_the_kernels(name):
    from fastmax_experiments_amd import adapter_v2 as av2
    from test_adapter_v2_cpu import tensors
    d, m = load_golden(name)
    t = {k: v.cuda() for k, v in tensors(d, m).items()}
    y = av2.adapter_forward(t["z"], t["adapter_scale"], t["adapter_bias"])
    dz, dsc, dbi = av2.adapter_backward(t["dy"], t["z"], t["adapter_scale"], t["adapter_bias"])
    assert y.dtype == t["y"].dtype and torch.equal(y, t["y"]), name
    assert torch.equal(dz, t["dz"]), name
    r = ar.restate(t["z"], t["adapter_scale"], t["adapter_bias"], t["dy"])
    assert ar.within(dsc, r["dscale64"], r["allow_scale"]) and ar.within(dbi, r["dbias64"], r["allow_bias"]), name


# ---- 2. the module ------------------------------------------------------------------------------------------------------------------
def _layer(K, N, dt, seed, bias=True):
    from fastmax_experiments_amd import adapter_v2 as av2
    torch.manual_seed(seed)
    lin = av2.AdapterV2Linear(K, N, bias=bias)
    with torch.no_grad():
        lin.adapter_scale.normal_(1.0, 0.3)
        lin.adapter_bias.normal_(0.0, 0.3)
    lin.fused = True
    return lin.to("cuda", dt)


def test_gradients_reach_exactly_the_inputs_that_ask_and_no_grad_saves_nothing(monkeypatch):
    from fastmax_experiments_amd import adapter_v2 as av2
    lin = _layer(32, 24, torch.bfloat16, 1)
    lin.linear.requires_grad_(False)
    x, gy = _rand((2, 5, 32), 2, torch.bfloat16), _rand((2, 5, 24), 3, torch.bfloat16)
    asked = []
    real = av2.adapter_backward
    monkeypatch.setattr(av2, "adapter_backward", lambda *a, **kw: (asked.append((kw["want_dz"], kw["want_param_grads"])), real(*a, **kw))[1])
    # everything frozen: no node at all
    y = lin(x)
    assert y.grad_fn is None and not y.requires_grad
    ref = av2.adapter_forward(lin.linear(x), lin.adapter_scale, lin.adapter_bias)
    assert torch.equal(y, ref)
    # x alone
    xx = x.clone().requires_grad_(True)
    lin(xx).backward(gy)
    assert asked == [(True, False)] and xx.grad is not None and lin.adapter_scale.grad is None and lin.adapter_bias.grad is None
    # one parameter alone: the sums, no dz (the frozen linear needs no gradient)
    lin.adapter_bias.requires_grad_(True)
    lin(x).backward(gy)
    assert asked[-1] == (False, True) and lin.adapter_bias.grad is not None and lin.adapter_scale.grad is None
    assert lin.adapter_bias.grad.dtype == torch.bfloat16
    # all of them
    lin.adapter_scale.requires_grad_(True)
    lin.linear.weight.requires_grad_(True)
    lin.zero_grad()
    lin(xx).backward(gy)
    assert asked[-1] == (True, True) and lin.linear.weight.grad is not None and lin.adapter_scale.grad is not None
    with pytest.raises(RuntimeError, match="once_differentiable"):  # a cotangent that itself depends on xx
        g, = torch.autograd.grad((lin(xx).float() ** 2).sum(), xx, create_graph=True)
        g.sum().backward()
    n = len(asked)
    with torch.no_grad():
        y = lin(xx)
    assert y.grad_fn is None and torch.equal(y, ref) and len(asked) == n
    lin.fused = False                                                # the tensor-op form gives the same bits
    assert torch.equal(lin(x), ref)


@pytest.mark.parametrize("dq", [False, True], ids=["nf4", "nf4_dq"])
def test_nf4_base_is_nf4linear_then_the_kernel(dq):
    from fastmax_experiments_amd import adapter_v2 as av2
    from fastmax_experiments_amd.lora import NF4Linear
    lin = _layer(128, 64, torch.bfloat16, 4).quantize_base(double_quant=dq)
    assert isinstance(lin.linear, NF4Linear) and lin.linear.double_quant == dq
    x = _rand((3, 7, 128), 5, torch.bfloat16).requires_grad_(True)
    lin.adapter_scale.requires_grad_(True), lin.adapter_bias.requires_grad_(True)
    y = lin(x)
    z = lin.linear(x.detach())
    assert torch.equal(y, av2.adapter_forward(z, lin.adapter_scale, lin.adapter_bias))
    gy = _rand((3, 7, 64), 6, torch.bfloat16)
    y.backward(gy)
    dz, dsc, dbi = av2.adapter_backward(gy, z, lin.adapter_scale, lin.adapter_bias)
    assert torch.equal(lin.adapter_scale.grad, dsc.to(torch.bfloat16)) and torch.equal(lin.adapter_bias.grad, dbi.to(torch.bfloat16))
    zz = x.detach().clone().requires_grad_(True)
    lin.linear(zz).backward(dz)
    assert torch.equal(x.grad, zz.grad)


# ---- 3. whole blocks ------------------------------------------------------------------------------------------------------------------
def _adapted_block(kind, alg, seed):
    from fastmax_experiments_amd import adapter_v2 as av2
    from fastmax_experiments_amd.block import Block
    from fastmax_experiments_amd.neox_block import NeoXBlock
    torch.manual_seed(seed)
    blk = (Block if kind == "block" else NeoXBlock)(n_embd=64, n_head=4, intermediate_size=88, attn_alg=alg, r=0)
    holder = torch.nn.ModuleList([blk])
    assert av2.adapt(holder) == (5 if kind == "block" else 4)
    with torch.no_grad():
        for n, p in blk.named_parameters():
            if n.endswith("adapter_scale") or (n.startswith("norm_") and n.endswith("weight")):
                p.normal_(1.0, 0.2)
            elif n.endswith("adapter_bias") or (n.startswith("norm_") and n.endswith("bias")):
                p.normal_(0.0, 0.2)
            p.requires_grad_(True)
    blk.fused_neighbours = True
    return blk.to("cuda", torch.bfloat16)


def _set_fused(module, on):
    from fastmax_experiments_amd import adapter_v2 as av2
    for m in module.modules():
        if isinstance(m, av2.AdapterV2Linear):
            m.fused = on


@pytest.mark.parametrize("alg", ["fastmax", "linearmax"])
@pytest.mark.parametrize("kind", ["block", "neox"])
def test_adapted_block_kernels_on_against_off(kind, alg, monkeypatch):
    from fastmax_experiments_amd import adapter_v2 as av2
    from fastmax_experiments_amd.attention_block import build_rope_cache
    blk = _adapted_block(kind, alg, 11)
    B, T, C = 2, 9, 64
    x, gy = _rand((B, T, C), 12, torch.bfloat16), _rand((B, T, C), 13, torch.bfloat16)
    cos, sin = build_rope_cache(T, blk.attn.rope_n_elem, device="cuda")
    layers = {n: m for n, m in blk.named_modules() if isinstance(m, av2.AdapterV2Linear)}
    by_scale = {m.adapter_scale.data_ptr(): n for n, m in layers.items()}
    sums, seen = {}, {}
    real = av2.adapter_backward

    def recording(dy, z, scale, bias, **kw):                         # the kernel's float32 sums, before the parameter-dtype cast
        out = real(dy, z, scale, bias, **kw)
        sums[by_scale[scale.data_ptr()]] = (out[1], out[2])
        return out

    monkeypatch.setattr(av2, "adapter_backward", recording)
    hooks = []
    for n, m in layers.items():                                      # z and dy of every adapted layer, from the kernels-off run
        hooks.append(m.linear.register_forward_hook(lambda mod, inp, out, n=n: seen.setdefault(n, {}).__setitem__("z", out.detach())))
        hooks.append(m.register_forward_hook(
            lambda mod, inp, out, n=n: out.register_hook(lambda g, n=n: seen[n].__setitem__("dy", g.detach())) and None))
    res = []
    for on in (False, True):
        _set_fused(blk, on)
        if on:
            for h in hooks:
                h.remove()
        blk.zero_grad()
        xx = x.clone().requires_grad_(True)
        y = blk(xx, cos, sin)
        y.backward(gy)
        res.append((y.detach(), xx.grad.clone(), {n: p.grad.clone() for n, p in blk.named_parameters()}))
    assert len(sums) == len(layers) == len(seen)
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    for n, g in res[0][2].items():
        if "adapter_" not in n:
            assert float(g.abs().max()) > 0 and torch.equal(g, res[1][2][n]), n              # norms and linears: the same bits
    for n, m in layers.items():
        N = seen[n]["z"].shape[-1]
        z, dy = seen[n]["z"].reshape(-1, N), seen[n]["dy"].reshape(-1, N)
        r = ar.restate(z, m.adapter_scale.detach(), m.adapter_bias.detach(), dy)
        dsc, dbi = sums[n]
        print(f"{kind} {alg} {n}: dscale {ar.worst(dsc, r['dscale64'], r['allow_scale']):.3f}, "
              f"dbias {ar.worst(dbi, r['dbias64'], r['allow_bias']):.3f} of the allowance")
        assert ar.within(dsc, r["dscale64"], r["allow_scale"]) and ar.within(dbi, r["dbias64"], r["allow_bias"]), n
        assert torch.equal(res[1][2][n + ".adapter_scale"], dsc.to(torch.bfloat16)), n
        assert torch.equal(res[1][2][n + ".adapter_bias"], dbi.to(torch.bfloat16)), n


# ---- 4. generation and the head -------------------------------------------------------------------------------------------------------
def test_generate_on_two_adapted_blocks_gives_the_same_tokens_with_kernels_on_and_off():
    from fastmax_experiments_amd import adapter_v2 as av2, generate
    from fastmax_experiments_amd.attention_block import build_rope_cache
    from fastmax_experiments_amd.block import Block
    from fastmax_experiments_amd.decode import FastmaxDecodeState
    torch.manual_seed(21)
    B, T, n_max, V, C = 2, 9, 14, 515, 128
    blocks = torch.nn.ModuleList(Block.from_config("pythia-14m", attn_alg="fastmax", r=0, intermediate_size=88) for _ in range(2))
    head = generate.NextTokenHead(C, V)
    model = torch.nn.ModuleDict(dict(blocks=blocks, head=head))
    assert av2.adapt(model) == 11
    with torch.no_grad():
        for n, p in model.named_parameters():
            if n.endswith("adapter_scale"):
                p.normal_(1.0, 0.2)
            elif n.endswith("adapter_bias"):
                p.normal_(0.0, 0.2)
    model.to("cuda").eval()
    wte = _rand((V, C), 22, torch.float32)
    prompt = torch.randint(0, V, (B, T), generator=torch.Generator().manual_seed(23)).cuda()
    cos, sin = build_rope_cache(n_max, blocks[0].attn.rope_n_elem, device="cuda")
    tokens = []
    for on in (True, False):
        _set_fused(blocks, on)
        states = [FastmaxDecodeState(B, 4, 32, "cuda", p=2, n_query_groups=4) for _ in range(2)]
        tokens.append(generate.generate(wte, list(blocks), head, states, prompt, n_max, cos=cos, sin=sin, temperature=0.0))
    assert tokens[0].shape == (B, n_max) and torch.equal(tokens[0][:, :T], prompt)
    assert torch.equal(tokens[0], tokens[1])


@pytest.mark.parametrize("form", ["dense", "biased", "nf4"])
def test_adapted_head_is_the_adapter_on_the_last_row_logits(form):
    from fastmax_experiments_amd import adapter_v2 as av2, generate
    torch.manual_seed(31)
    C, P, V = 128, 520, 515
    head = generate.NextTokenHead(C, P, V, lm_head_bias=form == "biased")
    if form == "biased":
        with torch.no_grad():
            head.lm_head.bias.normal_(0.0, 0.3)
    head.to("cuda", torch.bfloat16)
    if form == "nf4":
        head.quantize_base()
    plain = copy.deepcopy(head)
    assert av2.adapt(head) == 1 and isinstance(head.lm_head, av2.AdapterV2Linear) and head.lm_head.adapter_scale.shape == (P,)
    with torch.no_grad():
        head.lm_head.adapter_scale.normal_(1.0, 0.3)
        head.lm_head.adapter_bias.normal_(0.0, 0.3)
    x = _rand((3, 5, C), 32, torch.bfloat16)
    scores = plain.logits(x)
    assert scores.dtype == torch.float32 and scores.shape == (3, V)
    want = head.lm_head.adapter_scale.detach()[:V].float() * (scores + head.lm_head.adapter_bias.detach()[:V].float())
    got = head.logits(x)
    assert got.dtype == torch.float32 and torch.equal(got, want)
    assert torch.equal(head.logits(x), want)                         # the cached cast
    head.fused = False                                                 # the tensor-op head: the reference's roundings, close by
    eager = head.logits(x).detach()
    assert eager.shape == (3, V) and float((eager - want).abs().max()) < 0.05 * float(want.abs().max())


# ---- 5. the fine-tune step ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("optimizer", ["torch", "flat"])
def test_finetune_step_moves_exactly_the_trainable_parameters(optimizer, monkeypatch):
    from fastmax_experiments_amd import adapter_v2 as av2, finetune_step
    monkeypatch.setattr(av2, "FUSED_DEFAULT", True)                  # the step builds its own model: the kernels through the default
    made = []
    prepare = finetune_step.AttentionStack.prepare

    def recording(self, *a, **kw):
        out = prepare(self, *a, **kw)
        made.append((self, {n: p.detach().clone() for n, p in self.named_parameters()}))
        return out

    monkeypatch.setattr(finetune_step.AttentionStack, "prepare", recording)
    torch.manual_seed(0)
    r = finetune_step.run("pythia-14m", 1, "fastmax", seq=64, micro_batch=2, accum=1, steps=1, warmup=0,
                          device=torch.device("cuda"), optimizer=optimizer, method="adapter_v2")
    assert r["optimizer_steps"] == 1 and torch.isfinite(torch.tensor(r["last_loss"]))
    (model, before), = made
    assert all(m.fused for m in model.modules() if isinstance(m, av2.AdapterV2Linear))
    trainable = {n for n, p in model.named_parameters() if p.requires_grad}
    assert trainable == {f"blocks.0.{lin}.adapter_{p}" for lin in ("attn", "proj") for p in ("scale", "bias")}
    assert r["trainable_params"] == sum(before[n].numel() for n in trainable)
    for n, p in model.named_parameters():
        assert torch.equal(p.detach(), before[n]) != (n in trainable), n
