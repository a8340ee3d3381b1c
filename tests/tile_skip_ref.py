"""numpy restatement of the tile-skipping rule of the level-0 stride-1 layers (csrc/tile_skip.hip).

act: bool[H, W], the active pixels of the sparse first conv (H, W multiples of 16).
  blocks(act)      B_1 bool[H/4, W/4]: the block's 6x6 input window (pixels 4b-1 .. 4b+4, clipped to the image) meets act
  dilate(B)        3x3 block dilation: B_k from B_{k-1}
  tile_flags(act)  bool[3, H/16, W/16]: the tile holds no B_k block (k = 1, 2, 3) = skippable
  tile_class(..)   4 edge bits (1 top row, 2 bottom row, 4 left column, 8 right column): interior, 4 edges, 4 corners
  lists(flags_k)   items [(tile, mult)] and fills [(dst, src)] of one frame and layer, ascending in tile: per class the first
                   skippable tile is the representative (computed, mult = the class's skippable count), the others are filled from it;
                   a tile that is not skippable is an item with mult 1"""
import numpy as np

TILE, BLK = 16, 4
LAYERS = 3


def active_from_coors(coors, gx, gy):
    """Output pixels (gx/2 x gy/2) of the 3x3 stride-2 padding-1 first conv that see a pillar; coors int[n, >=2] = (cx, cy)."""
    H, W = gx // 2, gy // 2
    occ = np.zeros((gx + 2, gy + 2), bool)
    if len(coors):
        occ[np.asarray(coors)[:, 0] + 1, np.asarray(coors)[:, 1] + 1] = True
    act = np.zeros((H, W), bool)
    for ky in range(3):
        for kx in range(3):
            act |= occ[ky:ky + 2 * H:2, kx:kx + 2 * W:2]
    return act


def blocks(act):
    H, W = act.shape
    assert H % TILE == 0 and W % TILE == 0
    pad = np.zeros((H + 2, W + 2), bool)
    pad[1:-1, 1:-1] = act
    b = np.zeros((H // BLK, W // BLK), bool)
    for dy in range(BLK + 2):
        for dx in range(BLK + 2):
            b |= pad[dy:dy + H:BLK, dx:dx + W:BLK][:H // BLK, :W // BLK]
    return b


def dilate(b):
    pad = np.zeros((b.shape[0] + 2, b.shape[1] + 2), bool)
    pad[1:-1, 1:-1] = b
    out = np.zeros_like(b)
    for dy in range(3):
        for dx in range(3):
            out |= pad[dy:dy + b.shape[0], dx:dx + b.shape[1]]
    return out


def tile_flags(act):
    b = blocks(act)
    n = TILE // BLK
    out = []
    for k in range(LAYERS):
        if k:
            b = dilate(b)
        out.append(~b.reshape(b.shape[0] // n, n, b.shape[1] // n, n).any(axis=(1, 3)))
    return np.stack(out)


def tile_class(ty, tx, nty, ntx):
    return (1 if ty == 0 else 0) | (2 if ty == nty - 1 else 0) | (4 if tx == 0 else 0) | (8 if tx == ntx - 1 else 0)


def lists(flags_k, border=True):
    """items, fills of one frame and layer.  border=False: interior tiles only (edge and corner tiles are always computed)."""
    nty, ntx = flags_k.shape
    cls = np.array([[tile_class(ty, tx, nty, ntx) for tx in range(ntx)] for ty in range(nty)]).reshape(-1)
    skip = flags_k.reshape(-1).copy()
    if not border:
        skip &= cls == 0
    rep, cnt = {}, {}
    for t in np.flatnonzero(skip):
        c = int(cls[t])
        rep.setdefault(c, int(t))
        cnt[c] = cnt.get(c, 0) + 1
    items, fills = [], []
    for t in range(nty * ntx):
        c = int(cls[t])
        if not skip[t]:
            items.append((t, 1))
        elif rep[c] == t:
            items.append((t, cnt[c]))
        else:
            fills.append((t, rep[c]))
    return items, fills


def skip_fraction(flags_k, border=True):
    """Share of the tiles that are skippable (the issue's table; one representative per class is still computed)."""
    nty, ntx = flags_k.shape
    if border:
        return float(flags_k.mean())
    cls = np.array([[tile_class(ty, tx, nty, ntx) for tx in range(ntx)] for ty in range(nty)])
    return float((flags_k & (cls == 0)).sum()) / flags_k.size
