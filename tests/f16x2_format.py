"""The AVS_F16X2 storage format restated in plain torch (hi = fp16(x), lo = fp16(x - hi), runs of 8 hi halves then 8 lo
halves): no project code, no device needed.  test_gpu_f16x2.py checks the library's conversion kernels against it bit
for bit; the *_inputs modules build their operands and decode results with it."""
import torch


def emu_pack(x):
    """fp32 [..., C] (C % 8 == 0) -> float32-typed tensor of the same shape holding the AVS_F16X2 slots."""
    x = x.float().contiguous()
    c = x.shape[-1]
    assert c % 8 == 0
    xc = x.clamp(-65504.0, 65504.0)
    hi = xc.half()
    lo = (xc - hi.float()).half()
    runs = torch.stack([hi.reshape(-1, 8), lo.reshape(-1, 8)], 1).contiguous()   # [runs, 2, 8] halves = 32 bytes
    return runs.view(torch.float32).reshape(x.shape)


def emu_unpack(p):
    runs = p.contiguous().view(torch.float16).reshape(-1, 2, 8).float()
    return (runs[:, 0] + runs[:, 1]).reshape(p.shape)
