"""Run a fixed set of kNN launches through the C ABI and save the results: run once per library build (WM_HIP_LIB
selects it) and compare the files (kernel-restructuring changes that must give identical results; the exact rescoring
of wm_knn_topk has a fixed order, so its results are deterministic).

    WM_HIP_LIB=<build A> python tools/probes/knn_bitexact_probe.py a.pt
    WM_HIP_LIB=<build B> python tools/probes/knn_bitexact_probe.py b.pt
    python tools/probes/knn_bitexact_probe.py --compare a.pt b.pt      # exit status 1 if any entry differs

The table reaches every instantiation of csrc/knn.hip (which shape reaches which kernel: profiles/knn_refactor.md).
Every wm_knn_topk shape runs on two banks: n = 129 (one full chunk plus a one-row tail; with rows of one or two slabs
that is fewer ring steps than stages) and one on which every slice takes more ring steps than the ring has stages and the last chunk is ragged; k <= 8 with
both selection forms (WM_KNN_SELECT_THREADS unset and 256)."""
import ctypes
import os
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))


def compare(pa, pb):
    a, b = torch.load(pa), torch.load(pb)
    bad = [k for k in sorted(set(a) | set(b))
           if k not in a or k not in b or not (torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k])]
    print(f"{len(a)} / {len(b)} entries, {sum(torch.is_tensor(v) for v in a.values())} tensors, {len(bad)} differ")
    for k in bad:
        print("DIFFERS:", k)
    return 1 if bad else 0


if len(sys.argv) == 4 and sys.argv[1] == "--compare":
    sys.exit(compare(sys.argv[2], sys.argv[3]))

from ssl_wafermap_amd import _lib  # noqa: E402
from ssl_wafermap_amd import functional as F  # noqa: E402
from ssl_wafermap_amd._lib import check, dtype_code, ptr  # noqa: E402

lib = _lib.load()
st = torch.cuda.current_stream().cuda_stream
g = torch.Generator(device="cuda").manual_seed(0)
out = {}
os.environ.pop("WM_KNN_SELECT_THREADS", None)


def features(rows, d, dtype):
    return torch.nn.functional.normalize(torch.randn(rows, d, generator=g, device="cuda"), dim=1).to(dtype).contiguous()


def topk(q, bank, k, index_base=0):
    nq, d = q.shape
    n = bank.shape[0]
    need = lib.wm_knn_topk_workspace_bytes(nq, n, d, k)
    assert need > 0, (nq, n, d, k)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    sim = torch.empty(nq, k, device="cuda")
    idx = torch.empty(nq, k, device="cuda", dtype=torch.int32)
    check(lib.wm_knn_topk(ptr(q), ptr(bank), nq, n, d, dtype_code(q), k, index_base, ptr(sim), ptr(idx), ptr(ws), need, st),
          "wm_knn_topk")
    return sim.cpu(), idx.cpu()


# (dtype, d, nq, k, large bank): the kernel each one reaches is tabulated in profiles/knn_refactor.md
bf, f32 = torch.bfloat16, torch.float32
CASES = [(bf, 128, 64, 8, 262235), (bf, 128, 256, 8, 100003), (bf, 128, 40, 16, 262235),
         (bf, 256, 100, 8, 100003), (bf, 512, 64, 5, 50021), (bf, 256, 100, 16, 100003),
         (f32, 64, 96, 8, 150001), (f32, 128, 96, 8, 100003), (f32, 128, 33, 8, 100003), (f32, 512, 64, 5, 30011),
         (f32, 128, 64, 10, 100003)]
for dtype, d, nq, k, big in CASES:
    for n in (129, big):
        bank = features(n, d, dtype)
        q = features(nq, d, dtype)
        q[:min(nq, n) // 2] = bank[:min(nq, n) // 2]  # half of the queries are bank rows
        tag = f"{str(dtype).split('.')[-1]}_d{d}_nq{nq}_k{k}_n{n}"
        out["sim_" + tag], out["idx_" + tag] = topk(q, bank, k, index_base=7)
        if k <= 8:
            os.environ["WM_KNN_SELECT_THREADS"] = "256"
            out["sim256_" + tag], out["idx256_" + tag] = topk(q, bank, k, index_base=7)
            del os.environ["WM_KNN_SELECT_THREADS"]
        del bank, q

# wm_knn_topk_many: 5 batches of 64 queries over three lanes
bank = features(100003, 128, bf)
qq = features(5 * 64 - 10, 128, bf)
sim, idx = F.knn_topk_batched(qq, bank, 8, batch=64, lanes=3)
out["many_sim"], out["many_idx"] = sim.cpu(), idx.cpu()

# wm_knn_merge (k = 5: the 8-wide lists, k = 16), wm_knn_vote on its result
for k in (5, 16):
    parts = [topk(qq[:70], bank[o:o + 30000].contiguous(), k, index_base=o) for o in (0, 30000, 60000)]
    ps = torch.stack([p[0] for p in parts]).cuda()
    pi = torch.stack([p[1] for p in parts]).cuda()
    ms, mi = F.knn_merge(ps, pi)
    out[f"merge_sim_k{k}"], out[f"merge_idx_k{k}"] = ms.cpu(), mi.cpu()
    labels = torch.randint(0, 9, (90000,), generator=g, device="cuda")
    pred, scores = F.knn_vote(ms, mi, labels, 9, 0.1, return_scores=True)
    out[f"vote_pred_k{k}"], out[f"vote_scores_k{k}"] = pred.cpu(), scores.cpu()

# return codes of the unsupported corners (none of them launches)
q32, b32 = features(8, 512, f32), features(300, 512, f32)
ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
sim = torch.empty(8, 16, device="cuda")
idx = torch.empty(8, 16, device="cuda", dtype=torch.int32)


def rc(q, b, d, dt, k, w=None, wbytes=None):
    w = ptr(ws) if w is None else w
    return lib.wm_knn_topk(q, b, 8, 300, d, dt, k, 0, ptr(sim), ptr(idx), w, ws.numel() if wbytes is None else wbytes, st)


out["ws_k17"] = lib.wm_knn_topk_workspace_bytes(8, 300, 128, 17)
out["ws_f32_d512_k16"] = lib.wm_knn_topk_workspace_bytes(8, 300, 512, 16)
out["ws_f32_d512_k8"] = lib.wm_knn_topk_workspace_bytes(8, 300, 512, 8)
out["rc_k17"] = rc(ptr(q32), ptr(b32), 128, dtype_code(q32), 17)
out["rc_f32_d512_k16"] = rc(ptr(q32), ptr(b32), 512, dtype_code(q32), 16)
out["rc_misaligned_query"] = rc(ctypes.c_void_p(q32.data_ptr() + 4), ptr(b32), 128, dtype_code(q32), 8)
out["rc_misaligned_workspace"] = rc(ptr(q32), ptr(b32), 128, dtype_code(q32), 8, w=ctypes.c_void_p(ws.data_ptr() + 8))
out["rc_small_workspace"] = rc(ptr(q32), ptr(b32), 128, dtype_code(q32), 8, wbytes=64)
out["rc_d_not_a_slab"] = rc(ptr(q32), ptr(b32), 96, dtype_code(q32), 8)
assert all(out[k] != 0 for k in out if k.startswith("rc_")), {k: out[k] for k in out if k.startswith("rc_")}

torch.cuda.synchronize()
torch.save(out, sys.argv[1])
print(f"saved {len(out)} entries to {sys.argv[1]}")
