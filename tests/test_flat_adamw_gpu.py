"""optim.FlatAdamW on the device (csrc/flat_adamw.hip): parity of the float32 parameters and the masters with the float64
restatement (flat_adamw_ref.py) over mixed float32 / bfloat16 / float16 parameters, both access routes, float32 and bfloat16
buckets; then the exact claims -- 16-bit parameter == rounded master, run-to-run and segmentation-independent bits, the zeroed
bucket, a recorded step replayed with a changing device lr, the skipped non-finite step -- and one optimizer step behind the
DataParallelStepper against the torch route."""
import itertools

import numpy as np
import pytest
import torch

from flat_adamw_ref import PARITY_TOL, AdamWRef

pytestmark = pytest.mark.gpu

CHUNK = 1024                                                   # asserted against the library in _build
PACKED = [1, 7, 64, 1023, 1025, 4099, 3 * CHUNK + 5]           # packed offsets 0, 1, 8, 72, 1095, ...: the element route
FRIENDLY = [4, 8, 64, 1024, 1028, 4100, 3 * CHUNK + 8]         # whole pieces everywhere: the vector route
MIXED = [torch.float32, torch.bfloat16, torch.float16, torch.float32, torch.bfloat16, torch.float32, torch.bfloat16]
STEPS = 6


def _init(sizes, dtypes, seed=0):
    """|p| <= 0.4, already rounded to each parameter's dtype (host tensors)"""
    g = torch.Generator().manual_seed(seed)
    return [((torch.rand(s, generator=g) - 0.5) * 0.8).to(dt) for s, dt in zip(sizes, dtypes)]


def _grads(n, steps=STEPS, seed=1, scale=0.1):
    g = torch.Generator().manual_seed(seed)
    out = torch.randn(steps, n, generator=g) * scale
    out[:, ::97] = 0.0                                         # a few exactly-zero gradients (m = v = 0: the update is 0 / eps)
    out[1:, 5::211] = 0.0                                      # ... and some that are zero after a non-zero first step
    return out


def _build(init, bucket_dtype=torch.float32, **kw):
    from fastmax_experiments_amd import dp, optim
    assert optim.chunk_elems() == CHUNK
    params = [torch.nn.Parameter(w.clone().cuda()) for w in init]
    bucket = dp.FlatGradBucket(params, dtype=bucket_dtype)
    return optim.FlatAdamW(bucket, **kw)


def _state(opt):
    """every tensor a step writes, as host copies"""
    torch.cuda.synchronize()
    out = [opt.m.cpu(), opt.v.cpu()] + [p.detach().cpu() for p in opt.bucket.params]
    return out + ([] if opt.master is None else [opt.master.cpu()])


def _same_bits(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and torch.equal(x, y) for x, y in zip(a, b))


CONFIGS = list(itertools.product((0.0, 0.01), (1.0, 0.5), (None, "clips", "does not clip")))


@pytest.mark.parametrize("bucket_dtype", [torch.float32, torch.bfloat16], ids=["bucket_f32", "bucket_bf16"])
@pytest.mark.parametrize("sizes", [PACKED, FRIENDLY], ids=["packed", "friendly"])
def test_parity_with_the_float64_restatement(sizes, bucket_dtype):
    n = sum(sizes)
    init = _init(sizes, MIXED)
    grads = _grads(n).cuda()
    p0 = torch.cat([w.float() for w in init]).numpy()
    worst = 0.0
    for wd, grad_scale, clip in CONFIGS:
        # |g| = 0.1 sqrt(n) ~ 10 (5 after grad_scale 0.5): 1.0 clips every step, 1e3 never
        max_norm = {None: None, "clips": 1.0, "does not clip": 1e3}[clip]
        opt = _build(init, bucket_dtype, lr=1e-2, weight_decay=wd)
        vec, elem = opt.route_counts()
        if sizes is FRIENDLY:
            assert elem == 0 and vec == sum(-(-s // CHUNK) for s in sizes)
        else:
            assert elem > vec >= 1                              # only the 64-element segment at offset 8 is whole pieces
        ref = AdamWRef(p0, lr=1e-2, weight_decay=wd)
        for g in grads:
            opt.bucket.flat.copy_(g)
            fed = opt.bucket.flat.double().cpu().numpy()        # the bucket's own rounded values
            opt.step(grad_scale=grad_scale, max_norm=max_norm)
            ref.step(fed, grad_scale=grad_scale, max_norm=max_norm)
            if clip is not None:
                assert (ref.coef < 1.0) == (clip == "clips")
        assert opt.step_count() == STEPS and opt.skipped() == 0
        assert float(opt.bucket.flat.abs().sum()) == 0.0
        if clip is not None:
            assert opt.last_norm() == pytest.approx(ref.norm, rel=1e-5)
        assert np.abs(ref.p).max() <= 0.5
        off = 0
        for p in opt.bucket.params:
            k = p.numel()
            got = p.detach() if p.dtype == torch.float32 else opt.master[off:off + k]
            err = float(np.abs(got.double().cpu().numpy() - ref.p[off:off + k]).max())
            worst = max(worst, err)
            assert err <= PARITY_TOL, (wd, grad_scale, clip, off, err)
            if p.dtype != torch.float32:
                # a 16-bit parameter is round_to_nearest_even(master), bit for bit
                assert torch.equal(p.detach(), opt.master[off:off + k].to(p.dtype)), (wd, grad_scale, clip, off)
            else:
                assert float(opt.master[off:off + k].abs().sum()) == 0.0      # no master behind a float32 parameter
            off += k
    print(f"max |error| against the restatement: {worst:.3e} (bound {PARITY_TOL:.0e})")


def test_two_runs_give_identical_bits():
    init, grads = _init(PACKED, MIXED), _grads(sum(PACKED), 3).cuda()
    runs = []
    for _ in range(2):
        opt = _build(init, lr=1e-2)
        for g in grads:
            opt.bucket.flat.copy_(g)
            opt.step(grad_scale=0.5, max_norm=1.0)
        runs.append(_state(opt) + [torch.tensor(opt.last_norm())])
    assert _same_bits(*runs)


@pytest.mark.parametrize("max_norm", [None, 1.0], ids=["no_clip", "clip"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["params_f32", "params_bf16"])
def test_bits_do_not_depend_on_the_segmentation(dtype, max_norm):
    """the same flat data as one segment (vector route), as the packed sizes (element route, ragged chunks) and as the packed
    sizes in reverse order: m, v and the flat view of the weights are the same bits"""
    n = sum(PACKED)
    flat_init = _init([n], [dtype])[0]
    grads = _grads(n, 3).cuda()
    results = []
    for sizes in ([n], PACKED, PACKED[::-1]):
        opt = _build(list(torch.split(flat_init, sizes)), lr=1e-2)
        for g in grads:
            opt.bucket.flat.copy_(g)
            opt.step(max_norm=max_norm)
        torch.cuda.synchronize()
        weights = torch.cat([p.detach().reshape(-1) for p in opt.bucket.params]).cpu()
        results.append([opt.m.cpu(), opt.v.cpu(), weights] + ([] if opt.master is None else [opt.master.cpu()]))
    assert _same_bits(results[0], results[1]) and _same_bits(results[0], results[2])
    assert not torch.equal(results[0][2], flat_init)                  # it did move


def test_zero_grad_leaves_the_bucket_zero_and_the_views_aliased():
    opt = _build(_init(PACKED, [torch.float32] * len(PACKED)), lr=1e-2)
    bucket = opt.bucket
    loss = sum((p * p).sum() for p in bucket.params)
    loss.backward()                                                    # autograd accumulates into the views
    assert float(bucket.flat.abs().sum()) > 0
    kept = bucket.flat.clone()
    opt.step(zero_grad=False)
    assert torch.equal(bucket.flat, kept)
    opt.step()
    assert float(bucket.flat.abs().sum()) == 0.0
    off = 0
    for p in bucket.params:
        assert p.grad is not None and p.grad.data_ptr() == bucket.flat.data_ptr() + 4 * off
        off += p.numel()
    assert opt.step_count() == 2


def test_recorded_step_with_a_device_lr_equals_eager_steps():
    """step(lr=tensor) recorded once (one straight-line graph: the norm pass, the update pass) and replayed three times with the
    gradient and the lr changed between replays == three eager steps, bit for bit; the step counter advanced on the device"""
    init, grads = _init(PACKED, MIXED), _grads(sum(PACKED), 3).cuda()
    lrs = [1e-2, 5e-3, 2e-2]
    eager = _build(init, lr=1.0)
    lr_e = torch.zeros((), dtype=torch.float32, device="cuda")
    for g, lr in zip(grads, lrs):
        eager.bucket.flat.copy_(g)
        lr_e.fill_(lr)
        eager.step(max_norm=1.0, lr=lr_e)
    by_value = _build(init, lr=1.0)
    for g, lr in zip(grads, lrs):
        by_value.bucket.flat.copy_(g)
        by_value.param_groups[0]["lr"] = lr
        by_value.step(max_norm=1.0)
    assert _same_bits(_state(eager), _state(by_value))                # lr by pointer == the same float32 lr by value
    rec = _build(init, lr=1.0)
    lr_r = torch.zeros((), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rec.step(max_norm=1.0, lr=lr_r)
    assert rec.step_count() == 0                                       # recording runs nothing
    for g, lr in zip(grads, lrs):
        rec.bucket.flat.copy_(g)
        lr_r.fill_(lr)
        graph.replay()
    assert rec.step_count() == eager.step_count() == 3
    assert _same_bits(_state(eager), _state(rec))
    assert float(rec.bucket.flat.abs().sum()) == 0.0


@pytest.mark.parametrize("max_norm", [None, 1.0], ids=["no_clip", "clip"])
def test_skip_nonfinite_leaves_everything_but_the_gradient(max_norm):
    init, grads = _init(PACKED, MIXED), _grads(sum(PACKED), 3).cuda()
    opt = _build(init, lr=1e-2, skip_nonfinite=True)
    opt.bucket.flat.copy_(grads[0])
    opt.step(max_norm=max_norm)
    before = _state(opt)
    bad = grads[1].clone()
    bad[1100] = float("inf")                                           # one inf, in the middle of an element-route chunk
    opt.bucket.flat.copy_(bad)
    opt.step(max_norm=max_norm)
    assert _same_bits(before, _state(opt))
    assert opt.step_count() == 1 and opt.skipped() == 1 and float(opt.bucket.flat.abs().sum()) == 0.0
    opt.bucket.flat.copy_(grads[2])                                    # the next finite step goes through as step 2
    opt.step(max_norm=max_norm)
    assert opt.step_count() == 2 and opt.skipped() == 1 and not _same_bits(before, _state(opt))
    plain = _build(init, lr=1e-2)
    for g in (grads[0], grads[2]):
        plain.bucket.flat.copy_(g)
        plain.step(max_norm=max_norm)
    assert _same_bits(_state(plain), _state(opt))                      # as if the skipped step had not been there


def test_counter_advances_once_per_step_with_more_workgroups_than_ticket_slots():
    """71 + 1 chunks: the first-level ticket slots (64) have two members or one; the step counter still moves by exactly one per
    launch, a skipped step moves the skipped counter instead, and the values are the restatement's"""
    sizes, dtypes = [70 * CHUNK + 3, 5], [torch.float32, torch.bfloat16]
    init, grads = _init(sizes, dtypes), _grads(sum(sizes), 4).cuda()
    opt = _build(init, lr=1e-2, skip_nonfinite=True)
    assert sum(opt.route_counts()) == 72
    ref = AdamWRef(torch.cat([w.float() for w in init]).numpy(), lr=1e-2)
    for i, g in enumerate(grads[:3]):
        opt.bucket.flat.copy_(g)
        opt.step(max_norm=1.0)
        ref.step(g.double().cpu().numpy(), max_norm=1.0)
        assert opt.step_count() == i + 1 and opt.skipped() == 0
    bad = grads[3].clone()
    bad[-1] = float("nan")
    opt.bucket.flat.copy_(bad)
    opt.step(max_norm=1.0)
    assert opt.step_count() == 3 and opt.skipped() == 1
    got = torch.cat([opt.bucket.params[0].detach(), opt.master[-5:]]).double().cpu().numpy()
    assert float(np.abs(got - ref.p).max()) <= PARITY_TOL            # 3 steps: inside the 6-step bound


def test_state_dict_resumes_bit_for_bit_on_the_device():
    init, grads = _init(PACKED, MIXED), _grads(sum(PACKED), 4).cuda()
    a = _build(init, lr=1e-2)
    for g in grads[:2]:
        a.bucket.flat.copy_(g)
        a.step(max_norm=1.0)
    state, weights = a.state_dict(), [p.detach().cpu() for p in a.bucket.params]
    for g in grads[2:]:
        a.bucket.flat.copy_(g)
        a.step(max_norm=1.0)
    b = _build(weights, lr=1e-2)
    b.load_state_dict(state)
    for g in grads[2:]:
        b.bucket.flat.copy_(g)
        b.step(max_norm=1.0)
    assert b.step_count() == 4 and _same_bits(_state(a), _state(b))


def test_moved_parameter_storage_is_refused():
    opt = _build(_init([64, 7], [torch.float32, torch.bfloat16]))
    opt.bucket.params[1].data = opt.bucket.params[1].data.clone()
    with pytest.raises(RuntimeError, match="storage moved"):
        opt.step()


def test_stepper_with_flat_adamw_matches_the_torch_route():
    """one optimizer step (two micro-batches) of DataParallelStepper on the small attention stack: FlatAdamW (gather, no
    all-reduce at world 1, one fused pass with max_norm) against clip_grad_norm_ + torch.optim.AdamW + bucket.zero().  The
    kernels of the model are deterministic, so both routes see the same gradient bits; both optimizers are float32 AdamW, each
    within the restatement's bound of the exact update, so within PARITY_TOL of each other (one step: 6x inside the bound)."""
    from fastmax_experiments_amd import dp, finetune_step
    from fastmax_experiments_amd.attention_block import build_rope_cache
    from fastmax_experiments_amd.optim import FlatAdamW
    dev = torch.device("cuda")
    T, mb, accum = 256, 2, 2
    g = torch.Generator(device=dev).manual_seed(5)
    x = torch.randn(accum, mb, T, 128, device=dev, generator=g).to(torch.bfloat16)
    tgt = torch.randint(0, 512, (accum, mb, T), device=dev, generator=g)
    finals = []
    for route in ("torch", "flat"):
        torch.manual_seed(0)
        model = finetune_step.AttentionStack("pythia-14m", 2, "fastmax", vocab=512, lora_dropout=0.0).prepare(dev)
        cos, sin = (t.to(torch.bfloat16) for t in build_rope_cache(T, model.rope_n_elem, device=dev))
        params = dp.trainable_lora_parameters(model)
        opt = FlatAdamW(dp.FlatGradBucket(params), lr=1e-2) if route == "flat" else torch.optim.AdamW(params, lr=1e-2)
        st = dp.DataParallelStepper(model, opt, dp.TrainArgs(global_batch_size=mb * accum, micro_batch_size=mb, max_norm=1e-2),
                                    lambda m, b: m.loss(b[0], b[1], cos, sin))
        start = torch.cat([p.detach().float().reshape(-1) for p in params]).clone()
        for i in range(accum):
            st.micro_step((x[i], tgt[i]))
        assert st.step_count == 1 and float(st.bucket.flat.abs().sum()) == 0.0
        assert all(p.grad is not None and p.grad.data_ptr() == v.data_ptr() for p, v in zip(params, st.bucket._views))
        finals.append(torch.cat([p.detach().float().reshape(-1) for p in params]).clone())
        assert float((finals[-1] - start).abs().max()) > 1e-3         # it did step
    assert float(finals[0].abs().max()) <= 0.5
    err = float((finals[0].double() - finals[1].double()).abs().max())
    print(f"stepper: max |torch route - flat route| = {err:.3e}")
    assert err <= PARITY_TOL
