"""MNIST CNN — the Gaia paper's Exp. 6 workload (paper p.7 Figs. 11-12) on CPU: architecture size,
learnable synthetic data, the capturable AdamW against the eager one, and the best-vs-worst harness
with two 2-rank gloo jobs on a fake 8-device node."""
import json
import os
import socket
import subprocess
import sys

import torch

from gpu_topology_on_k8s_amd.models import FlatAdamW
from gpu_topology_on_k8s_amd.models.mnist import MnistCNN, MnistConfig

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_architecture_matches_the_pytorch_example():
    cfg = MnistConfig.named("mnist-cnn")
    assert cfg.num_params() == 1_199_882  # torchvision/examples mnist/main.py Net
    assert cfg.pooled == 9216
    m = MnistCNN(cfg, device="cpu")
    x, y = m.synthetic_batch(4, torch.Generator().manual_seed(0))
    assert x.shape == (4, 1, 28, 28) and x.dtype == torch.bfloat16 and x.is_contiguous(memory_format=torch.channels_last)
    assert m(x).shape == (4, 10) and 0 <= int(y.min()) and int(y.max()) < 10
    # identical replicas from the same seed (DP ranks), different data per generator seed
    assert torch.equal(MnistCNN(cfg, device="cpu").flat.data, m.flat.data)
    x2, _ = m.synthetic_batch(4, torch.Generator().manual_seed(1))
    assert not torch.equal(x, x2)


def test_capturable_adamw_matches_eager_on_cpu():
    cfg = MnistConfig()
    a, b = MnistCNN(cfg, device="cpu", seed=1), MnistCNN(cfg, device="cpu", seed=1)
    oa, ob = FlatAdamW(a.flat, lr=1e-3), FlatAdamW(b.flat, lr=1e-3, capturable=True)
    g = torch.Generator().manual_seed(3)
    for _ in range(3):
        grad = (torch.randn(a.flat.numel, generator=g) * 0.1).to(torch.bfloat16)
        a.flat.grad.copy_(grad)
        b.flat.grad.copy_(grad)
        oa.step(grad_scale=0.5)
        ob.step(grad_scale=0.5)
    assert oa.t == ob.t == 3 and float(ob.t_dev) == 3.0
    # bias corrections in fp32 on the device vs double on the host: master agrees to fp32 rounding,
    # the bf16 weights to at most one ulp at rounding boundaries
    assert torch.allclose(oa.master, ob.master, atol=1e-6)
    assert torch.allclose(a.flat.data.float(), b.flat.data.float(), rtol=8e-3, atol=1e-6)
    ob.t = 7  # checkpoint restore sets the device counter too
    assert float(ob.t_dev) == 7.0


def test_mnist_training_learns_on_cpu():
    from gpu_topology_on_k8s_amd.models.train import train

    env = {k: os.environ.get(k) for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    try:
        with socket.socket() as sk:  # a fixed port collides with other tests under pytest -n
            sk.bind(("127.0.0.1", 0))
            os.environ["MASTER_PORT"] = str(sk.getsockname()[1])
        out = train("mnist-cnn", batch=32, steps=25, warmup=1, device_kind="cpu", log=False, lr=1e-3)
    finally:
        import torch.distributed as dist

        if dist.is_initialized():
            dist.destroy_process_group()
        for k, v in env.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    assert out["throughput_unit"] == "images/s" and out["images_per_s"] > 0 and out["tokens_per_s"] is None
    assert out["epoch_s"] == 60000 / out["images_per_s"] and out["graph"] is False
    assert out["loss_first"] > 2.0 and out["loss_last"] < 0.5 * out["loss_first"]


def _rel64(a, b):
    return float((a - b).abs().max() / b.abs().max())


def test_conv_reference_matches_library_conv_and_autograd():
    """models/mnist_ref.py (shifted matrix products, explicit pooling stack) against F.conv2d +
    F.max_pool2d + autograd in float64, random continuous inputs (no ties) and a random keep mask."""
    import torch.nn.functional as F

    from gpu_topology_on_k8s_amd.models import mnist_ref as R

    g = torch.Generator().manual_seed(11)
    B, p = 3, 0.25
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    x, w1, b1, w2, b2, dp = rnd(B, 28, 28), rnd(32, 3, 3), rnd(32), rnd(64, 3, 3, 32) * 0.1, rnd(64), rnd(B, 12, 12, 64)
    keep = torch.rand(B, 12, 12, 64, generator=g) < 0.7
    h1, pooled, code = R.conv_stack_ref(x, w1, b1, w2, b2, keep, p)
    gw1, gb1, gw2, gb2 = R.conv_stack_grads_ref(x, h1, w2, code, dp, p)

    P = [t.clone().requires_grad_(True) for t in (w1, b1, w2, b2)]
    a1 = F.relu(F.conv2d(x[:, None], P[0][:, None], P[1]))
    a2 = F.relu(F.conv2d(a1, P[2].permute(0, 3, 1, 2), P[3]))
    want = F.max_pool2d(a2, 2).permute(0, 2, 3, 1) * keep / (1 - p)
    want.backward(dp)
    assert _rel64(h1, a1.detach().permute(0, 2, 3, 1)) < 1e-10
    assert _rel64(pooled, want.detach()) < 1e-10
    for name, got, t in zip(("conv1.w", "conv1.b", "conv2.w", "conv2.b"), (gw1, gb1, gw2, gb2), P):
        assert got.shape == t.grad.shape, name
        assert _rel64(got, t.grad) < 1e-10, (name, _rel64(got, t.grad))
    # the code byte: keep bit = the mask given, pos bit = the pooled value is live, argmax = the pixel
    # that holds the window's maximum
    assert torch.equal((code >> 3) & 1, keep.to(torch.uint8))
    pos = ((code >> 2) & 1).bool()
    assert torch.equal(pos & keep, pooled > 0) and 0.3 < float(pos.float().mean()) < 1.0
    pre = a2.detach().permute(0, 2, 3, 1)  # [B,24,24,64]
    am = (code & 3).long()
    py, px = torch.meshgrid(torch.arange(12), torch.arange(12), indexing="ij")
    picked = pre[torch.arange(B)[:, None, None, None], (2 * py + 0)[None, :, :, None] + (am >> 1),
                 (2 * px)[None, :, :, None] + (am & 1), torch.arange(64)[None, None, None, :]]
    assert torch.equal(picked[pos], F.max_pool2d(a2, 2).detach().permute(0, 2, 3, 1)[pos])


def test_conv_reference_tie_picks_the_first_pixel_in_kernel_order():
    """A window whose four conv2 outputs are equal, and one whose maximum sits at q = 1 and q = 2:
    the reference picks the first maximum in the order q = 2*(y&1) + (x&1), as the kernel's ``>``."""
    from gpu_topology_on_k8s_amd.models import mnist_ref as R

    # conv1 = identity tap (centre weight 1 on channel 0), conv2 = centre tap of channel 0 into co 0:
    # conv2's output pixel (y, x) of channel 0 is x[y+2, x+2]
    w1, b1 = torch.zeros(32, 3, 3), torch.zeros(32)
    w1[0, 1, 1] = 1.0
    w2, b2 = torch.zeros(64, 3, 3, 32), torch.zeros(64)
    w2[0, 1, 1, 0] = 1.0
    x = torch.zeros(1, 28, 28)
    x[0, 2:4, 2:4] = 3.0                       # window (0,0): all four equal -> q = 0
    x[0, 2, 4], x[0, 2, 5], x[0, 3, 4], x[0, 3, 5] = 1.0, 5.0, 5.0, 2.0   # window (0,1): q = 1 and 2 tie -> 1
    x[0, 4, 2], x[0, 4, 3], x[0, 5, 2], x[0, 5, 3] = 1.0, 2.0, 4.0, 4.0   # window (1,0): q = 2 and 3 tie -> 2
    keep = torch.ones(1, 12, 12, 64, dtype=torch.bool)
    h1, pooled, code = R.conv_stack_ref(x, w1, b1, w2, b2, keep, 0.5)
    assert [int(code[0, 0, 0, 0]), int(code[0, 0, 1, 0]), int(code[0, 1, 0, 0])] == [0 | 12, 1 | 12, 2 | 12]
    assert [float(pooled[0, 0, 0, 0]), float(pooled[0, 0, 1, 0]), float(pooled[0, 1, 0, 0])] == [6.0, 10.0, 8.0]
    assert int(code[0, 5, 5, 0]) == 8 and int(code[0, 0, 0, 1]) == 8  # all-zero window: argmax 0, not positive
    # the gradient goes to that one pixel only
    dp = torch.zeros(1, 12, 12, 64)
    dp[0, 0, 1, 0] = 1.0
    *_, extra = R.conv_stack_grads_ref(x, h1, w2, code, dp, 0.5, with_intermediates=True)
    assert float(extra["dy2"].abs().sum()) == 2.0 and float(extra["dy2"][0, 0, 3, 0]) == 2.0


def test_dropout_keep_fraction_and_p_zero():
    from gpu_topology_on_k8s_amd.models.mnist_ref import dropout_keep

    n = 1_000_000
    k = dropout_keep(0x7F4A7C15, 7.0, n, 0.5)
    assert k.dtype == torch.bool and k.shape == (n,)
    assert abs(float(k.float().mean()) - 0.5) < 0.01
    assert bool(dropout_keep(0x7F4A7C15, 7.0, n, 0.0).all())
    assert not torch.equal(k, dropout_keep(0x7F4A7C15, 8.0, n, 0.5))           # the step matters
    assert not torch.equal(k, dropout_keep(0x7F4A7C15 ^ 0x5BD1E995, 7.0, n, 0.5))  # and the seed
    assert torch.equal(k, dropout_keep(0x7F4A7C15 + (1 << 32), 7.0, n, 0.5))   # seed mod 2^32
    assert torch.equal(k[:1000], dropout_keep(0x7F4A7C15, 7.0, 1000, 0.5))     # indexed, not sequential


def test_head_references_match_autograd():
    import torch.nn.functional as F

    from gpu_topology_on_k8s_amd.models import mnist_ref as R

    g = torch.Generator().manual_seed(12)
    z = torch.randn(37, 10, generator=g, dtype=torch.float64) * 3
    lab = torch.randint(0, 10, (37,), generator=g)
    zz = z.clone().requires_grad_(True)
    want = F.cross_entropy(zz, lab)
    want.backward()
    loss, dlog = R.xent10_ref(z, lab)
    assert abs(float(loss) - float(want.detach())) < 1e-12 and _rel64(dlog, zz.grad) < 1e-10
    h = torch.randn(37, 128, generator=g, dtype=torch.float64)
    keep = torch.rand(37, 128, generator=g) < 0.5
    dy = torch.randint(-3, 4, (37, 128), generator=g).double()
    hh = h.clone().requires_grad_(True)
    yw = F.relu(hh) * keep / 0.5
    yw.backward(dy)
    y, mask = R.relu_dropout_ref(h, keep, 0.5)
    dh, gb = R.relu_dropout_bwd_ref(dy, mask, 0.5)
    assert torch.equal(y, yw.detach()) and torch.equal(dh, hh.grad) and torch.equal(gb, hh.grad.sum(0))


def test_mnist_best_vs_worst_harness_cpu(tmp_path):
    out = tmp_path / "r.json"
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench", "train_llama.py"), "--gpus", "2", "--device", "cpu",
                        "--discovery", "fake", "--model", "mnist-cnn", "--batch", "16", "--steps", "3", "--warmup", "1",
                        "--out", str(out)], capture_output=True, text=True, timeout=600, cwd=REPO, env=dict(env, GTK_FAKE_GPUS="8"))
    assert p.returncode == 0, p.stderr[-4000:]
    s = json.loads(out.read_text())["summary"]
    assert s["throughput_unit"] == "images/s" and s["best_throughput"] > 0 and s["worst_throughput"] > 0
    assert s["best_devices"] != s["worst_devices"] and s["best_epoch_s"] > 0 and s["seq_len"] is None
