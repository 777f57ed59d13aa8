"""Record the fused stem backward (wm_bn_relu_maxpool_bwd) of the build in use as golden arrays for tests/test_gpu_stem_pool.py.

    [WM_HIP_LIB=<library of the revision to record>] python tools/probes/stem_pool_golden.py [out_dir]

Run it on the revision whose results are to be KEPT (the parent of a change to bn_pool_bwd_apply), never on the code under
test.  Per shape (N, C, H, W, G) it stores the seeded inputs (y, gamma, beta, pooled gradient), what the forward half hands
to the backward (window positions, selected inputs, batch mean / invstd) and the backward's dy, dgamma, dbeta, as
tests/golden/stem_pool/n<N>c<C>h<H>w<W>g<G>_<name>.npy (bf16 tensors as their uint16 patterns)."""
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
SHAPES = [(2, 16, 12, 12, 1), (4, 64, 20, 24, 2)]
DEV = "cuda:0"


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def main(out_dir):
    from ssl_wafermap_amd import _lib

    lib, ptr = _lib.load(), _lib.ptr
    out_dir.mkdir(parents=True, exist_ok=True)
    for n, c, h, w, g in SHAPES:
        gen = torch.Generator().manual_seed(1000 + c)
        y = (torch.randn(n, h, w, c, generator=gen) * 2 + 0.3).bfloat16().to(DEV)       # NHWC
        gamma = torch.rand(c, generator=gen) + 0.5
        gamma[::5] *= -1                                                                # some channels flip the ReLU side
        beta = torch.randn(c, generator=gen) * 0.2
        p, q = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        pdy = torch.randn(n, p, q, c, generator=gen).bfloat16().to(DEV)
        gamma, beta = gamma.to(DEV), beta.to(DEV)
        rows = n * h * w
        ws = torch.empty(lib.wm_bn_workspace_bytes(rows, c, g), dtype=torch.uint8, device=DEV)
        mean, invstd, scale, shift = (torch.empty((g, c), dtype=torch.float32, device=DEV) for _ in range(4))
        rm, rv = torch.zeros(c, device=DEV), torch.ones(c, device=DEV)
        st = _lib.stream_ptr()
        _lib.check(lib.wm_bn_train_stats(ptr(y), ptr(gamma), ptr(beta), ptr(rm), ptr(rv), 0, rows, c, g, 1e-5, 0.1, ptr(mean),
                                         ptr(invstd), ptr(scale), ptr(shift), 0, 0, ptr(ws), ws.numel(), st), "stats")
        out = torch.empty((n, p, q, c), dtype=torch.bfloat16, device=DEV)
        idx = torch.empty((n, p, q, c), dtype=torch.uint8, device=DEV)
        ysel = torch.empty_like(out)
        _lib.check(lib.wm_bn_relu_maxpool3x3s2_fwd(ptr(y), ptr(scale), ptr(shift), n, h, w, c, g, ptr(out), ptr(idx), ptr(ysel),
                                                   st), "fwd")
        dy = torch.empty_like(y)
        dgamma, dbeta = torch.empty(c, device=DEV), torch.empty(c, device=DEV)
        _lib.check(lib.wm_bn_relu_maxpool_bwd(ptr(y), ptr(ysel), ptr(pdy), ptr(idx), n, h, w, c, ptr(gamma), ptr(beta), ptr(mean),
                                              ptr(invstd), g, ptr(dgamma), ptr(dbeta), 0, ptr(dy), ptr(ws), ws.numel(), st), "bwd")
        torch.cuda.synchronize()
        tag = f"n{n}c{c}h{h}w{w}g{g}"
        for name, arr in (("y", bits(y)), ("pooled_dy", bits(pdy)), ("ysel", bits(ysel)), ("dy", bits(dy)),
                          ("idx", idx.cpu().numpy()), ("gamma", gamma.cpu().numpy()), ("beta", beta.cpu().numpy()),
                          ("mean", mean.cpu().numpy()), ("invstd", invstd.cpu().numpy()), ("dgamma", dgamma.cpu().numpy()),
                          ("dbeta", dbeta.cpu().numpy())):
            np.save(out_dir / f"{tag}_{name}.npy", arr)
        print(tag, "recorded; |dy| max", float(dy.float().abs().max()), "library", _lib.LIB_PATH)


if __name__ == "__main__":
    main(Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "tests" / "golden" / "stem_pool")
