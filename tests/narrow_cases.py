"""What the suites of the narrow gradient builds share (tests/test_conv_narrow_host.py, tests/test_conv_narrow_gpu.py): the shapes and a
restatement of the host-side plans of csrc/conv_narrow.hip.

Shapes are (B, Ci, Co, H, W, pad): the filter is (Co, Ci, 3, 3), H x W the map of x / dx, ``pad`` the FORWARD padding; dy is
(B, Co, H + 2 pad - 2, W + 2 pad - 2).

K11n (k_conv3x3_narrow_dgrad) tiles every image's dx in 8 rows x 16 columns; a workgroup of four waves takes a tile, wave w its rows
2 w and 2 w + 1, and walks tiles blockIdx, blockIdx + grid, ... with grid = min(tiles, 2048); Co / 32 channel groups are staged one after
the other.  K12n (k_conv3x3_narrow_wgrad) cuts the batch's M = B * Ho * Wo output pixels into S slices of ``pps`` pixels (a multiple of
32, at least 512, about M / 2048), one wave per slice, chunks of 32 pixels, every other chunk negated."""

DGRAD_TILE_H, DGRAD_TILE_W, DGRAD_MAX_GRID = 8, 16, 2048
WGRAD_SLICES, WGRAD_MIN_PPS = 2048, 512

DGRAD_SHAPES = [
    (1, 16, 32, 5, 7, 1),        # 35 pixels: one tile, rows 5..7 and columns 7..15 of it outside the image; wave 3 stores nothing
    (4, 16, 32, 8, 8, 1),        # four images = four tiles of exactly 8 rows, half of every tile's columns outside
    (1, 16, 32, 1, 257, 1),      # a one-row image: 17 tiles along x, the last with one live column; rows -1 and 1 outside for every pixel
    (3, 16, 64, 10, 10, 1),      # two channel groups (filter and tile staged twice per tile); two tiles along y, the second with 2 live rows
    (2, 16, 96, 7, 6, 0),        # pad 0: dy is 5 x 4, the product's padding 2: two halo rows / columns outside on every side; three groups
    (2, 16, 32, 3, 4, 2),        # pad 2: dy (5 x 6) larger than dx, the product's padding 0: the halo is all inside
    (5, 5, 32, 1, 1, 1),         # a 1 x 1 image: only the centre tap inside; eleven absent channels (zero filter rows, masked stores)
    (3, 16, 32, 42, 42, 1),      # the 84 x 84 encoder's block: 6 x 3 tiles an image, ragged last tile row (2 live rows) and column (10 live)
    (2, 16, 32, 64, 64, 1),      # the block itself: 8 x 4 full tiles an image
    (2100, 3, 32, 2, 2, 1),      # 2100 tiles > the grid of 2048: workgroups 0..51 walk a second tile with the filter kept in LDS
    (2, 16, 64, 20, 33, 1),      # 3 x 3 tiles, 17th column alone in a tile, with two channel groups
]

WGRAD_SHAPES = [
    (2, 16, 32, 4, 4, 1),        # M 32: one chunk; W = 4 with pad 1: every pixel touches an end of its row
    (3, 16, 32, 4, 4, 1),        # M 48: two chunks, the second half full and negated
    (2, 5, 24, 5, 5, 1),         # ragged Ci (45 of 144 columns) and Co (24 of 32 rows), odd width: M 50
    (1, 1, 1, 3, 4, 2),          # the smallest ragged case: one row, nine columns; pad 2, M 30
    (3, 16, 32, 2, 6, 2),        # pad 2: M 96, three full chunks (odd count: the last step of the pair loop is alone)
    (2, 16, 32, 6, 6, 0),        # pad 0: M 32
    (37, 16, 32, 12, 12, 1),     # M 5328: 11 slices of 512, the last 208 (6.5 chunks); slices begin inside images; W a multiple of 4
    (23, 16, 32, 17, 17, 0),     # M 5175: 11 slices of 512, the last 55 (two chunks, 23 pixels in the second); W no multiple of 4
    (3, 16, 32, 42, 42, 1),      # M 5292: 11 slices, the last 172
    (2, 16, 32, 64, 64, 1),      # M 8192: 16 full slices of 16 chunks
    (700, 7, 9, 50, 50, 1),      # M 1 750 000 > 2048 x 512: pps grows to 864 (27 chunks), S 2026, the last slice 400 pixels
]
# shape -> (S, pixels per slice, pixels of the last slice, chunks of a full slice, chunks of the last slice)
WGRAD_CLAIMS = {
    (2, 16, 32, 4, 4, 1): (1, 512, 32, 1, 1),
    (3, 16, 32, 4, 4, 1): (1, 512, 48, 2, 2),
    (2, 5, 24, 5, 5, 1): (1, 512, 50, 2, 2),
    (1, 1, 1, 3, 4, 2): (1, 512, 30, 1, 1),
    (3, 16, 32, 2, 6, 2): (1, 512, 96, 3, 3),
    (2, 16, 32, 6, 6, 0): (1, 512, 32, 1, 1),
    (37, 16, 32, 12, 12, 1): (11, 512, 208, 16, 7),
    (23, 16, 32, 17, 17, 0): (11, 512, 55, 16, 2),
    (3, 16, 32, 42, 42, 1): (11, 512, 172, 16, 6),
    (2, 16, 32, 64, 64, 1): (16, 512, 512, 16, 16),
    (700, 7, 9, 50, 50, 1): (2026, 864, 400, 27, 13),
}
# config 3's own minibatch: dy is exactly 2^32 bytes, x 2^31
CONFIG3 = (8192, 16, 32, 64, 64, 1)


def dgrad_plan(B, Ci, Co, H, W, pad):
    """aurppo_conv3x3_dgrad_narrow_f32's launch, restated: dict(tiles_y, tiles_x, tiles, grid, groups, wop_bytes)."""
    ty, tx = (H + DGRAD_TILE_H - 1) // DGRAD_TILE_H, (W + DGRAD_TILE_W - 1) // DGRAD_TILE_W
    tiles = B * ty * tx
    return dict(tiles_y=ty, tiles_x=tx, tiles=tiles, grid=min(tiles, DGRAD_MAX_GRID), groups=Co // 32, wop_bytes=(Co // 32) * 9 * 3 * 1024)


def wgrad_plan(B, Ci, Co, H, W, pad):
    """narrow_wgrad_plan of csrc/conv_narrow.hip, restated: dict(S, pps, last, chunks, chunks_last, M), or None where it refuses."""
    Ho, Wo = H + 2 * pad - 2, W + 2 * pad - 2
    if not (1 <= Ci <= 16 and 1 <= Co <= 32 and 0 <= pad <= 2 and B > 0 and H > 0 and W > 0 and Ho > 0 and Wo > 0):
        return None
    M, HoWo, HW = B * Ho * Wo, Ho * Wo, H * W
    pps = max((M + WGRAD_SLICES - 1) // WGRAD_SLICES, WGRAD_MIN_PPS)
    pps = (pps + 31) // 32 * 32
    per_img = 4 * max(HoWo * Co, HW * Ci)
    if per_img * 2 >= 1 << 31:
        return None

    def too_far(p):
        return (p // HoWo + 2) * per_img >= (1 << 31) or p + HoWo >= (1 << 23)
    while pps > 32 and too_far(pps):
        pps = (pps // 2 + 31) // 32 * 32
    if too_far(pps):
        return None
    S = (M + pps - 1) // pps
    if S > 1 << 20:
        return None
    last = M - (S - 1) * pps
    return dict(S=S, pps=pps, last=last, chunks=(min(pps, M) + 31) // 32, chunks_last=(last + 31) // 32, M=M)


def wgrad_slices_from_ws(ws_bytes, Ci, Co):
    assert ws_bytes > 0 and ws_bytes % (Co * Ci * 36) == 0
    return ws_bytes // (Co * Ci * 36)
