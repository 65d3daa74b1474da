"""LearnedSpikeLayer under DistributedDataParallel: two ranks share cuda:0 (spawned child processes, process group
over gloo, as tests/test_gpu_ddp.py), each with its own batch through ``TrainStep(distributed=True)`` of a spike
layer in front of a small conv3d head.  Checked: DDP reduces the log-intensity's gradient like any other float32
parameter -- both ranks hold the same gradients, equal to the mean of the two batches' single-process gradients --
and after three steps the replicas (the intensity included) are bit-identical and the intensity has moved.

Bar for the mean: the ranks run the arithmetic of the single-process passes on the same data, so only gloo's
float32 average and the conv library's choice of algorithm per process can differ: 1e-4 of each tensor's largest
gradient, two orders above float32 rounding of sums of this length, far below a missing or doubled reduction (a
factor of 2, or one rank's value instead of the mean)."""
import os
import socket
import sys
import tempfile

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "medical-vision-textural-bias_amd")
SHAPE = (2, 1, 16, 16, 16)
LOC = [(9, 7, 6)]


def _batch(rank: int, dev):
    g = torch.Generator().manual_seed(300 + rank)
    x = torch.randn(SHAPE, generator=g)
    lab = (torch.rand(SHAPE, generator=g) > 0.5).float()
    return x.to(dev), lab.to(dev)


def _net():
    from texbias.spikes import LearnedSpikeLayer

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.spike = LearnedSpikeLayer(8.0, seed=0)
            self.head = torch.nn.Conv3d(1, 1, 3, padding=1)

        def forward(self, x):
            return self.head(self.spike(x, loc=LOC))

    torch.manual_seed(0)
    return Net()


def _first_grads(step, x, lab):
    step.opt.zero_grad(set_to_none=True)
    step.loss_fn(step.model(x), lab).backward()
    return {n: p.grad.detach().clone().cpu() for n, p in step.module.named_parameters()}


def _rank_main(rank: int, world: int, port: int, out_dir: str):
    sys.path[:0] = [PKG, ROOT]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK="0")
    import torch.distributed as dist
    from texbias.train import TrainStep
    torch.backends.cudnn.benchmark = False
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    step = TrainStep(_net(), dev, distributed=True)
    x, lab = _batch(rank, dev)
    grads = _first_grads(step, x, lab)
    step.opt.step()
    for _ in range(2):
        step(x, lab)
    torch.cuda.synchronize()
    params = {n: p.detach().cpu() for n, p in step.module.named_parameters()}
    torch.save({"grads": grads, "params": params}, os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_ddp_reduces_the_intensity_gradient(gpu):
    import torch.multiprocessing as mp
    sys.path[:0] = [PKG, ROOT]
    from texbias.train import TrainStep
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    with tempfile.TemporaryDirectory() as td:
        ctx = mp.get_context("spawn")
        procs = [ctx.Process(target=_rank_main, args=(r, 2, port, td)) for r in range(2)]
        for p in procs:
            p.start()
        for p in procs:
            p.join(timeout=240)
        codes = [p.exitcode for p in procs]
        for p in procs:
            if p.is_alive():
                p.kill()
        assert codes == [0, 0], f"rank exit codes {codes}"
        r0 = torch.load(os.path.join(td, "rank0.pt"), weights_only=True)
        r1 = torch.load(os.path.join(td, "rank1.pt"), weights_only=True)
    assert "spike.log_intensity" in r0["grads"]
    for n in r0["grads"]:
        assert torch.equal(r0["grads"][n], r1["grads"][n]), n          # one reduced gradient on every replica
        assert torch.equal(r0["params"][n], r1["params"][n]), n        # replicas bit-identical after 3 steps
    assert float(r0["params"]["spike.log_intensity"]) != 8.0 and torch.isfinite(r0["params"]["spike.log_intensity"]).all()
    # the reduced gradient is the mean of the two batches' own gradients
    dev = torch.device("cuda", 0)
    single = TrainStep(_net(), dev)
    own = [_first_grads(single, *_batch(r, dev)) for r in range(2)]
    assert not torch.equal(own[0]["spike.log_intensity"], own[1]["spike.log_intensity"])
    for n, g in r0["grads"].items():
        mean = (own[0][n].double() + own[1][n].double()) / 2
        scale = max(own[0][n].abs().max().item(), own[1][n].abs().max().item())
        err = (g.double() - mean).abs().max().item()
        print(f"{n}: reduced {g.flatten()[:2].tolist()}  mean {mean.flatten()[:2].tolist()}  err / scale {err / scale:.2e}")
        assert err <= 1e-4 * scale, (n, err, scale)
