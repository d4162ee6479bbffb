"""What the host and the GPU tests of the range census of the 16-bit backbone share (addendum): the clip, the two copies of
the synthetic weights that leave fp16's range at one known place, and the fp32 value there, computed on the CPU by the oracle."""
import torch

from tests import helpers as H

HOT_BLOCK = "backbone.backward_1.main.2.rg.0."      # the first RCAB the first time step of the first branch runs
HOT_SCALE = 3.0e6                                   # on its second convolution: the residual stream leaves fp16's range, not bf16's
TAIL_SCALE = 3.0e6                                  # on conv_hr: its activation leaves fp16's range in the upsampling tail


def clip_u8(n, t, h, w, seed):
    from eavsr_amd.utils.synthetic import synthetic_clip
    big = synthetic_clip(n, t, h + (-h) % 4 + 4, w + (-w) % 4 + 4, seed=seed)
    return (big[..., :h, :w] * 255).round().to(torch.uint8).contiguous()


def state_dict(tag="x4", hot=None):
    """the synthetic weights; hot="block": HOT_BLOCK's second convolution scaled; hot="tail": conv_hr scaled"""
    sd = H.filled(H.model_shapes(tag), "trained_like")
    keys = {None: (), "block": (HOT_BLOCK + "res.2.weight", HOT_BLOCK + "res.2.bias"), "tail": ("conv_hr.weight", "conv_hr.bias")}[hot]
    for k in keys:
        sd[k] = sd[k] * (HOT_SCALE if hot == "block" else TAIL_SCALE)
    return sd


def hot_block_fp32(sd, last_frame):
    """the residual stream behind HOT_BLOCK at the branch's first time step, in fp32 on the CPU (oracle/eavsr_oracle.py): the encoder's
    features of the clip's last frame beside the zero state, the input convolution, the block"""
    import torch.nn.functional as F
    from oracle import eavsr_oracle as O
    with torch.no_grad():
        f = O.encoder(sd, "encoder.", last_frame)
        p = "backbone.backward_1."
        x = F.leaky_relu(F.conv2d(torch.cat([f, torch.zeros_like(f)], 1), sd[p + "main.0.weight"], sd[p + "main.0.bias"], 1, 1), 0.1)
        return O.rcab(sd, HOT_BLOCK, x)
