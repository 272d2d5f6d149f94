"""optim.FlatAdamW behind the DataParallelStepper on CPU ranks (the rehearsal path): world-size-2 gloo processes -- gather, ONE
all-reduce SUM without the division, `step(grad_scale=1/world, max_norm=...)` -- land on the parameters a single process gets
from the same global batch (the pattern of test_dp_gloo.py), and a single-process run with max_norm set equals the float64
restatement fed with the gradients the bucket held."""
import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from flat_adamw_ref import PARITY_TOL, AdamWRef
from test_dp_gloo import TinyLoRA, _data, _free_port, _loss

MAX_NORM = 0.5


def _stepper(model, world):
    from fastmax_experiments_amd import dp
    from fastmax_experiments_amd.optim import FlatAdamW
    params = dp.trainable_lora_parameters(model)
    opt = FlatAdamW(dp.FlatGradBucket(params), lr=1e-2)
    train = dp.TrainArgs(global_batch_size=16, micro_batch_size=2, max_norm=MAX_NORM)
    st = dp.DataParallelStepper(model, opt, train, _loss)
    assert st.bucket is opt.bucket and st.accum == 16 // world // 2
    return st, opt, params


def _run(rank, world, port, out):
    from fastmax_experiments_amd import dp
    if world > 1:
        dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    model = TinyLoRA()
    st, opt, params = _stepper(model, world)
    X, Y = _data()
    for s in range(X.shape[0]):
        xs, ys = dp.shard_batch(X[s], rank, world), dp.shard_batch(Y[s], rank, world)
        for m in range(st.accum):
            st.micro_step((xs[2 * m:2 * m + 2], ys[2 * m:2 * m + 2]))
    assert st.step_count == 3 and opt.step_count() == 3
    # what bucket.zero() leaves: an all-zero bucket and .grad views that alias it
    assert float(st.bucket.flat.abs().sum()) == 0.0 and model.lora_A.grad.data_ptr() == st.bucket.flat.data_ptr()
    if rank == 0:
        torch.save({k: v.detach().clone() for k, v in model.state_dict().items()}, out)
    if world > 1:
        flat = torch.cat([p.detach().flatten() for p in params])
        ref = flat.clone()
        dist.broadcast(ref, 0)
        assert torch.equal(flat, ref)                    # every rank holds identical parameters
        dist.destroy_process_group()


def test_flat_adamw_world2_matches_single_process(tmp_path):
    single, multi = str(tmp_path / "single.pt"), str(tmp_path / "multi.pt")
    _run(0, 1, 0, single)
    mp.spawn(_run, args=(2, _free_port(), multi), nprocs=2, join=True)
    a, b = torch.load(single), torch.load(multi)
    for k in a:
        assert torch.allclose(a[k], b[k], rtol=1e-5, atol=1e-6), k
    assert not torch.equal(a["lora_A"], TinyLoRA().lora_A)          # it did train
    assert torch.equal(a["base"], TinyLoRA().base)                   # frozen base untouched


def test_single_process_with_max_norm_equals_the_restatement():
    from fastmax_experiments_amd.optim import FlatAdamW

    fed = []

    class Recording(FlatAdamW):
        def step(self, **kw):
            fed.append((self.bucket.flat.double().numpy().copy(), kw))
            return super().step(**kw)

    from fastmax_experiments_amd import dp
    model = TinyLoRA()
    params = dp.trainable_lora_parameters(model)
    ref = AdamWRef(torch.cat([p.detach().reshape(-1) for p in params]).numpy(), lr=1e-2)
    opt = Recording(dp.FlatGradBucket(params), lr=1e-2)
    st = dp.DataParallelStepper(model, opt, dp.TrainArgs(global_batch_size=16, micro_batch_size=2, max_norm=MAX_NORM), _loss)
    X, Y = _data()
    for s in range(X.shape[0]):
        for m in range(st.accum):
            st.micro_step((X[s][2 * m:2 * m + 2], Y[s][2 * m:2 * m + 2]))
    assert len(fed) == 3
    clipped = []
    for g, kw in fed:
        assert kw == dict(grad_scale=1.0, max_norm=MAX_NORM, zero_grad=True)
        ref.step(g, **{k: v for k, v in kw.items() if k != "zero_grad"})
        clipped.append(ref.coef < 1.0)
    assert any(clipped)                                               # MAX_NORM does clip here
    got = torch.cat([p.detach().reshape(-1) for p in params]).double().numpy()
    assert np.abs(ref.p).max() <= 0.5
    assert float(np.abs(got - ref.p).max()) <= PARITY_TOL            # 3 steps: inside the 6-step bound


def test_finetune_step_run_takes_the_flat_optimizer():
    """`finetune_step.run(optimizer="flat")` on the CPU stand-in model: the same number of optimizer steps and a finite loss that
    is close to the torch route's (same batches, same hyper-parameters); an unknown name is refused"""
    import pytest
    from fastmax_experiments_amd import finetune_step
    dev = torch.device("cpu")
    res = {o: finetune_step.run("pythia-14m", 1, "fastmax", 8, 2, 2, 3, 1, dev, toy=True, optimizer=o) for o in ("torch", "flat")}
    assert res["flat"]["optimizer_steps"] == res["torch"]["optimizer_steps"] == 4
    assert res["flat"]["bucket_bytes"] == res["torch"]["bucket_bytes"]
    assert res["flat"]["last_loss"] == pytest.approx(res["torch"]["last_loss"], rel=1e-4)
    with pytest.raises(ValueError, match="optimizer should be"):
        finetune_step.run("pythia-14m", 1, "fastmax", 8, 2, 2, 1, 0, dev, toy=True, optimizer="sgd")
