"""bench.py --dump-outputs writer: float .npy files, a fixed seeded sample of
the optimizer's fp32 master parameters, identical from run to run (CPU, toy
model through the real ZeRO2Engine)."""

import numpy
import torch

import bench
from dolomite_engine_amd.zero import ZeRO2Engine

N_BIG = bench.DUMP_SAMPLE_PER_BUCKET * 3 + 7  # the bucket is larger than the sample


def _stepped_engine():
    """bf16 toy model built after the bench's weight seed, one AdamW step."""
    torch.manual_seed(bench.WEIGHT_SEED)
    model = torch.nn.Linear(N_BIG, 1).to(torch.bfloat16)
    engine = ZeRO2Engine(model, lr=1e-5, betas=(0.9, 0.95), eps=1e-10, weight_decay=0.1, bucket_mb=1)
    x = torch.randn(4, N_BIG, generator=torch.Generator().manual_seed(3)).to(torch.bfloat16)
    engine.zero_grad()
    engine.set_sync(True)
    model(x).float().pow(2).mean().backward()
    engine.step(lr=1e-5, grad_clip=1.0)
    return model, engine


def test_dump_outputs_is_float_npy_and_repeatable(tmp_path):
    steps = [(11.25, 0.5), (11.0, 0.75)]
    model, engine = _stepped_engine()
    bench.dump_outputs(str(tmp_path / "a"), steps, engine)
    _, engine_b = _stepped_engine()  # a second "run": same seed, same inputs
    bench.dump_outputs(str(tmp_path / "b"), steps, engine_b)

    names = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert names == ["grad_norm.npy", "loss.npy", "loss_per_step.npy", "params_sample.npy"]
    for name in names:
        a = numpy.load(tmp_path / "a" / name)
        b = numpy.load(tmp_path / "b" / name)
        assert a.dtype in (numpy.float32, numpy.float64), (name, a.dtype)
        numpy.testing.assert_array_equal(a, b)

    assert numpy.load(tmp_path / "a" / "loss.npy").tolist() == [11.0]
    assert numpy.load(tmp_path / "a" / "grad_norm.npy").tolist() == [0.75]
    assert numpy.load(tmp_path / "a" / "loss_per_step.npy").tolist() == [11.25, 11.0]

    # the sample is exactly master[idx] for the indices drawn from DUMP_SEED
    assert len(engine.buckets) == 1
    master = engine.buckets[0].master
    assert master.dtype == torch.float32 and master.numel() > bench.DUMP_SAMPLE_PER_BUCKET
    g = torch.Generator().manual_seed(bench.DUMP_SEED)
    idx = torch.randint(0, master.numel(), (bench.DUMP_SAMPLE_PER_BUCKET,), generator=g)
    sample = numpy.load(tmp_path / "a" / "params_sample.npy")
    numpy.testing.assert_array_equal(sample, master[idx].numpy())

    # and it reflects the optimizer step: the fp32 masters moved although
    # (nearly) no bf16 model value did
    bf16_copy = engine.buckets[0].flat_param[: master.numel()].float()
    assert (master != bf16_copy).float().mean() > 0.5
