"""The shapes tests/test_gpu_conv.py runs, each with the kernel instantiation it is there for (a WM_ROUTE_* code of
include/wafer_hip.h).  wm_conv2d_route is the arbiter: tests/test_abi.py asks it about every row on the CPU, and the
GPU tests ask again before they launch, so a predicate change that moves a shape to another kernel fails here instead
of silently leaving a kernel untested.

A shape is (N, C, H, W, K, R, stride, pad); `geom` makes the eleven geometry integers of the C ABI from it.  A stem
shape (C = 3, 7 x 7 / 2 / 3 on an image) becomes the 4 x 4 convolution over the space-to-depth image the kernels run."""
import kernel_check as kc


def geom(shape):
    n, c, h, w, k, r, stride, pad = shape
    if c == 3:
        return (n, h // 2, w // 2, 16, k, 4, 4, h // 2, w // 2, 1, 2)
    p, q = kc.conv_out_hw(h, w, r, r, stride, pad)
    return (n, h, w, c, k, r, r, p, q, stride, pad)


def linear_geom(rows, c, k):
    return (rows, 1, 1, c, k, 1, 1, 1, 1, 1, 0)


IG64, IG128 = (lambda *a, **kw: kc.route_igemm(64, *a, **kw)), (lambda *a, **kw: kc.route_igemm(128, *a, **kw))
PATCH_SHAPES = [(2, 64, 8, 8, 64, 3, 1, 1),      # every tile on every border
                (1, 64, 8, 16, 64, 3, 1, 1),     # the pair's tiles side by side
                (1, 64, 16, 8, 64, 3, 1, 1),     # ... stacked
                (2, 64, 8, 24, 64, 3, 1, 1),     # the middle pair straddles two images
                (2, 64, 24, 24, 64, 3, 1, 1)]    # 9 pairs, an interior tile
STEM_PATCH_SHAPES = [(2, 3, 16, 16, 64, 7, 2, 3), (1, 3, 16, 32, 64, 7, 2, 3), (2, 3, 48, 48, 64, 7, 2, 3)]
STEM_IGEMM_SHAPES = [(1, 3, 16, 16, 64, 7, 2, 3),    # one tile: an odd count
                     (1, 3, 48, 48, 64, 7, 2, 3),    # nine tiles
                     (1, 3, 18, 22, 64, 7, 2, 3)]    # space-to-depth 9 x 11: ragged

# ---- forward: (route, shape)
FWD = [(IG64(8, 0), (1, 64, 9, 11, 64, 3, 1, 1)),        # M = 99
       (IG64(8, 0), (1, 64, 11, 13, 64, 3, 1, 1)),       # M = 143 = 128 + 15
       (IG64(8, 0), (2, 128, 8, 8, 64, 3, 1, 1)),        # M = 128 exactly
       (IG64(8, 0), (1, 64, 8, 8, 64, 3, 1, 1)),         # one 8 x 8 tile, an odd count: the patch kernel's fallback
       (IG64(8, 0), (1, 64, 10, 10, 64, 3, 1, 0)),       # pad 0
       (IG64(8, 0), (1, 64, 9, 11, 192, 1, 1, 0)),       # three column tiles
       (IG128(8, 0), (2, 64, 16, 16, 128, 3, 2, 1)),     # M = 128
       (IG128(8, 0), (1, 128, 5, 7, 128, 1, 2, 0)),      # M = 12
       (IG128(8, 0), (3, 256, 14, 14, 512, 3, 2, 1))]    # M = 147
FWD += [(kc.route_patch(0), s) for s in PATCH_SHAPES]
FWD += [(kc.ROUTE_STEM_PATCH, s) for s in STEM_PATCH_SHAPES] + [(IG64(2, 0), s) for s in STEM_IGEMM_SHAPES]

# ---- forward with statistics slots: (route, shape, groups)
FWD_STATS = [(IG64(8, 0), (2, 128, 8, 8, 64, 3, 1, 1), 1),
             (IG128(8, 0), (4, 64, 16, 16, 128, 3, 2, 1), 2),
             (kc.route_patch(0), (4, 64, 8, 8, 64, 3, 1, 1), 2),
             (kc.route_patch(0), (2, 64, 8, 16, 64, 3, 1, 1), 2),
             (kc.ROUTE_STEM_PATCH, (4, 3, 16, 16, 64, 7, 2, 3), 2)]

# ---- input gradient, plain and with a shortcut gradient: (route, shape)
DGRAD = [(IG64(8, 3), (1, 64, 9, 11, 64, 3, 1, 1)),
         (IG128(8, 3), (2, 128, 8, 8, 64, 3, 1, 1)),     # 128-wide dx tile
         (IG64(8, 3), (1, 64, 9, 11, 192, 1, 1, 0)),
         (IG128(8, 3), (5, 512, 7, 7, 512, 3, 1, 1))]
DGRAD += [(kc.route_patch(1), s) for s in PATCH_SHAPES]
DGRAD += [(IG64(8, 2), (2, 64, 16, 16, 128, 3, 2, 1)),   # one tile per parity class
          (IG64(8, 2), (2, 64, 16, 16, 128, 1, 2, 0)),
          (IG64(8, 2), (4, 64, 16, 32, 128, 3, 2, 1)),   # four tiles per class
          (IG128(8, 1), (1, 128, 5, 7, 64, 3, 2, 1)),    # odd sides
          (IG128(8, 1), (1, 128, 5, 7, 64, 1, 2, 0)),
          (IG64(8, 1), (2, 64, 12, 12, 128, 3, 2, 1))]   # even sides, class size 72

# ---- input gradient with the BatchNorm-backward epilogue: (route, shape, groups)
DGRAD_BNB = [(IG128(8, 3, bnb=True), (2, 128, 8, 8, 128, 3, 1, 1), 1),
             (kc.route_patch(1, True), (2, 64, 8, 8, 64, 3, 1, 1), 1),
             (kc.route_patch(1, True), (4, 64, 8, 8, 64, 3, 1, 1), 2),
             (IG64(8, 2, bnb=True), (2, 64, 16, 16, 128, 3, 2, 1), 1),
             (IG64(8, 2, bnb=True), (4, 64, 16, 16, 128, 3, 2, 1), 2)]
BNB_REFUSED = (1, 128, 5, 7, 64, 3, 2, 1)               # odd sides: wm_conv2d_dgrad_bnstat_ok says 0

# ---- weight gradient: (route, geometry, splits or None)
WG = kc.route_wgrad
WGRAD = [(kc.ROUTE_WGRAD_PATCH64, geom(s), None) for s in ((1, 64, 8, 8, 64, 3, 1, 1), (3, 64, 8, 8, 64, 3, 1, 1),
                                                           (2, 64, 24, 24, 64, 3, 1, 1))]
WGRAD += [(WG(64, 8, 3), geom((1, 64, 9, 11, 64, 3, 1, 1)), None),     # two chunks, the second ragged at 35 pixels
          (WG(64, 8, 3), geom((2, 128, 8, 8, 64, 3, 1, 1)), None),
          (WG(64, 8, 3), linear_geom(37, 192, 64), None),              # Linear 192 -> 64, 37 rows
          (WG(64, 8, 1), geom((1, 128, 5, 7, 64, 1, 2, 0)), None),     # 12 pixels, less than one chunk
          (WG(128, 8, 3), geom((2, 64, 16, 16, 128, 3, 2, 1)), None),
          (WG(128, 8, 1), geom((2, 64, 16, 16, 128, 1, 2, 0)), None),
          (WG(128, 8, 2), geom((3, 256, 14, 14, 512, 1, 2, 0)), None),
          (WG(128, 8, 3), geom((8, 512, 7, 7, 512, 3, 1, 1)), 4)]      # 7 chunks in 4 splits of 2, 2, 2, 1
WGRAD_STEM = [(WG(64, 2, 4), s) for s in STEM_PATCH_SHAPES + STEM_IGEMM_SHAPES]
# the patch shapes with WM_WGRAD_PATCH=0 (read per call)
WGRAD_PATCH_OFF = [(WG(64, 8, 3), geom(s)) for s in ((1, 64, 8, 8, 64, 3, 1, 1), (3, 64, 8, 8, 64, 3, 1, 1),
                                                      (2, 64, 24, 24, 64, 3, 1, 1))]


def stem_loop_images(cus, per_cu=3, extra=5):
    """N 16 x 16 images = N / 2 tile pairs, a handful more than the stem kernel's resident blocks (per_cu per compute
    unit): one launch in which `extra` blocks loop over a second pair"""
    return 2 * (per_cu * cus + extra)
