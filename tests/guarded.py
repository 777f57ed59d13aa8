"""Sentinel-guarded device buffers for the GPU tests that call the C ABI directly: every output lies inside a larger buffer
filled with a sentinel, and finish() asserts the margins untouched, so that an overrun shows as a failed assertion."""
import math

import torch

DEV = "cuda:0"
MARGIN = 64             # sentinel elements on either side of every output

_SENTINEL = {torch.bfloat16: -7.0, torch.float32: -7777.0, torch.uint8: 0xA5, torch.int64: -99}


class Guarded:
    """A device tensor of `shape` inside a buffer with MARGIN sentinel elements on both sides"""
    live = []

    def __init__(self, shape, dtype, init=None):
        n = math.prod(shape)
        self.fill = _SENTINEL[dtype]
        self.whole = torch.full((n + 2 * MARGIN,), self.fill, dtype=dtype, device=DEV)
        self.t = self.whole[MARGIN:MARGIN + n].view(shape)
        assert self.t.data_ptr() % 16 == 0
        if init is not None:
            self.t.copy_(init.to(dtype))
        Guarded.live.append(self)

    @property
    def ptr(self):
        return self.t.data_ptr()

    def intact(self):
        return bool((self.whole[:MARGIN] == self.fill).all()) and bool((self.whole[-MARGIN:] == self.fill).all())


def finish(what):
    """synchronize, assert every margin of every buffer allocated since the last call"""
    torch.cuda.synchronize()
    bad = [tuple(g.t.shape) for g in Guarded.live if not g.intact()]
    Guarded.live = []
    assert not bad, f"{what}: wrote outside its outputs {bad}"


def ok(lib, rc, what):  # noqa: ARG001
    from ssl_wafermap_amd import _lib

    _lib.check(rc, what)


def stream():
    from ssl_wafermap_amd import _lib

    return _lib.stream_ptr()
