"""The small module tree of the optimiser fixture (tests/golden/make_optim_golden.py writes it, tests/test_gpu_optim.py and
tests/test_optim_host.py read it).  Its parameter sizes are the smallest at which csrc/optim_step.hip can still go wrong
(CHUNK = LIDAR_OPTIM_CHUNK = 1024 elements, one 256-thread workgroup, four elements per thread):
  * numel 1, 3, 5, 7: the scalar tail alone, and a vector group followed by a tail;
  * exactly one chunk, one chunk + 1, three chunks + 2;
  * a 64-element vector at a 4-byte storage offset: 4-byte but not 16-byte aligned, the scalar path for a whole tensor;
  * 72 BatchNorm vectors of 8 elements: more table entries than a wave has lanes (and the reference's second parameter group);
  * one 16-element tensor whose gradients are of order 1e-8: eps decides its update;
  * one 8 x 4 x 3 x 3 convolution weight.
"""
import torch
from torch import nn

CHUNK = 1024
N_BN = 36
TINY_GRAD = 1e-8


class Bag(nn.Module):
    """a leaf module holding bare parameters"""

    def __init__(self, shapes, device):
        super().__init__()
        for k, s in enumerate(shapes):
            self.register_parameter(f"p{k}", nn.Parameter(torch.zeros(s, device=device)))


class Offset(nn.Module):
    """a 64-element parameter that starts one float into its storage"""

    def __init__(self, device):
        super().__init__()
        self.register_buffer("flat", torch.zeros(68, device=device), persistent=False)
        self.p = nn.Parameter(self.flat[1:65])


class Net(nn.Module):
    def __init__(self, device="cpu"):
        super().__init__()
        self.tails = Bag([(1,), (3,), (5,), (7,)], device)
        self.chunks = Bag([(CHUNK,), (CHUNK + 1,), (3 * CHUNK + 2,)], device)
        self.offset = Offset(device)
        self.norms = nn.Sequential(*[nn.BatchNorm1d(8, device=device) for _ in range(N_BN)])
        self.tiny = Bag([(16,)], device)
        self.conv = nn.Conv2d(4, 8, 3, bias=False, device=device)


def reference_order(model):
    """the parameters in the order of the reference's optimizer (not BatchNorm, then BatchNorm), restated for the tests"""
    bn = [p for m in model.norms for p in m.parameters()]
    rest = ([p for p in model.tails.parameters()] + [p for p in model.chunks.parameters()] + [model.offset.p]
            + [p for p in model.tiny.parameters()] + [model.conv.weight])
    return rest + bn


def tiny_index(model):
    return [id(p) for p in reference_order(model)].index(id(model.tiny.p0))


def offset_index(model):
    return [id(p) for p in reference_order(model)].index(id(model.offset.p))


def split(flat, shapes):
    """a flat array -> per-tensor arrays of the stored shapes"""
    out, at = [], 0
    for s in shapes:
        n = 1
        for d in s:
            n *= d
        out.append(flat[..., at:at + n].reshape(flat.shape[:-1] + tuple(s)))
        at += n
    assert at == flat.shape[-1]
    return out
