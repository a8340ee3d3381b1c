"""GPU: what the training tests share.  The small geometries (an engine on 24 x 16 cells for the stateless primitives, a network on
GX x GY = 48 x 32 cells, level-2 map 6 x 4, with two frames of pillars), the two ways a gradient is judged (check_grad: the project's
bar for fixture gradients, 4 x the reference's own float32 deviation; check_bound: an element-wise a-priori bound) and the backward of
the whole RPN made by hand with the engine primitives.  A helper that differs from module to module stays in its module."""
import numpy as np
import pytest
import torch

from conftest import load_pkg
import blocktrain_ref as R

ENG = load_pkg("engine").Engine
CONV, NECK = ENG.RPN_CONV_KEYS, ENG.NECK_KEYS
GX, GY = 48, 32
_ENGINES = {}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def small_cfg(gx, gy, max_batch):
    cfg = load_pkg("synth").load_config("eight_20cm")
    cfg["detection_range"] = [0.0, 0.0, -2.5, 0.2 * gx, 0.2 * gy, 8.5]
    cfg["max_voxels"] = 2000
    cfg["device"] = torch.device("cuda:0")
    cfg["max_batch"] = max_batch
    return cfg


def engine(max_batch=3):
    """An engine without weights (pp_unit_backward is stateless and takes its map size from the call)."""
    if max_batch not in _ENGINES:
        load_pkg().install()
        _ENGINES[max_batch] = load_pkg("engine").Engine(small_cfg(24, 16, max_batch))
    return _ENGINES[max_batch]


@pytest.fixture(scope="module")
def loaded():
    """48 x 32 cells (level-2 map 6 x 4) with the seeded weights committed and a canvas with a few pillars."""
    load_pkg().install()
    synth = load_pkg("synth")
    eng = load_pkg("engine").Engine(small_cfg(48, 32, 2))
    sd = {k: np.asarray(v, np.float32) for k, v in synth.seeded_state_dict(0).items()}
    eng.load_state_dict(sd)
    rng = np.random.default_rng(3)
    canvas = np.zeros((1, 64, 48, 32), np.float32)
    cells = rng.choice(48 * 32, 300, replace=False)
    canvas[0, :, cells // 32, cells % 32] = np.maximum(rng.standard_normal((300, 64)), 0).astype(np.float32)
    return dict(eng=eng, sd=sd, canvas=dev(canvas))


def random_case(C, h, w, nb, seed):
    rng = np.random.default_rng(seed)
    u = R.tie_free(rng.standard_normal((nb, C, h, w)))
    assert not R.near_ties(u, 1e-4).any()
    wt = (rng.standard_normal((C, C, 3, 3)) * 0.05).astype(np.float32)
    dz = rng.standard_normal((nb, C, h, w)).astype(np.float32)
    dskip = rng.standard_normal((nb, C, h, w)).astype(np.float32)
    return u, wt, dz, dskip


def check_grad(got, want64, ref32_dev, scale, what):
    got = got.cpu().numpy().astype(np.float64).reshape(-1)
    bar = 4.0 * ref32_dev * scale
    err = np.abs(got - want64.reshape(-1)).max()
    print(f"{what}: max err {err:.3e}, bar {bar:.3e} ({err / bar:.2f} of it)")
    assert err <= bar, what


def check_bound(got, want, bound, what):
    frac = float((np.abs(got.cpu().numpy().astype(np.float64) - want) / bound).max())
    print(f"{what}: largest fraction of the a-priori bound {frac:.3f}")
    assert frac <= 1.0, (what, frac)


def small_net(seed=0):
    cfg = small_cfg(GX, GY, 4)
    load_pkg("framework.voxel_generator").VoxelGenerator(cfg)
    net = load_pkg("networks.pointpillars8_shared").PointPillars(cfg)
    net.load_state_dict(load_pkg("synth").seeded_state_dict(seed))
    return net, cfg


def two_frames(eng):
    rng = np.random.default_rng(4)
    frames = []
    for f in range(2):
        n = 200 + 60 * f
        cells = rng.choice(GX * GY, n, replace=False)
        coors = np.stack([cells // GY, cells % GY, np.zeros(n, np.int64)], 1).astype(np.int32)
        vox = rng.standard_normal((n, eng.T, eng.F)).astype(np.float32)
        frames.append(dict(voxels=vox, coordinates=coors, num_points_per_voxel=rng.integers(1, eng.T + 1, n).astype(np.int32)))
    utils = load_pkg("framework.utils")
    return utils.example_convert_to_torch(utils.merge_second_batch(frames))


def canvases_of(eng, example):
    coors = example["coordinates"]
    out = []
    for f in range(2):
        sel = coors[:, -1] == f
        c = coors[sel][:, :-1].contiguous()
        num = eng.num_tensor(c.shape[0])
        feat = eng.pfn(example["voxels"][sel].contiguous(), c, example["num_points_per_voxel"][sel].contiguous(), num)
        out.append(eng.scatter(feat, c, num))
    return out


def seeded_sd(seed=0):
    return {k: np.asarray(v, np.float32) for k, v in load_pkg("synth").seeded_state_dict(seed).items()}


def stacked_taps(eng, canvases):
    """backbone_train_taps per frame, stacked: y, (x1, x2, x3), per level the list of unit inputs [nb,C,h,w], (z1, z2, z3)."""
    outs = [eng.backbone_train_taps(c) for c in canvases]
    y = torch.cat([o[0] for o in outs])
    xs = [torch.cat([o[1][b] for o in outs]) for b in range(3)]
    units = [[torch.stack([o[2][b][k] for o in outs]) for k in range(ENG.RPN_UNITS[b])] for b in range(3)]
    zs = [torch.cat([o[3][b] for o in outs]) for b in range(3)]
    return y, xs, units, zs


def by_hand(eng, canvas, taps, p, gy, need_dx):
    """The backward of the whole RPN with the engine primitives, written out: -> ({key: dw}, dcanvas, {conv key: the (input, dy) the
    call saw})."""
    y, xs, units, zs = taps
    dw, seen = {}, {}
    dxn = []
    for b in range(3):
        dw[NECK[b]], dx = eng.neck_backward(b, xs[b], p[NECK[b]], y, gy, need_dx=True)
        dxn.append(dx)

    def unit(key, u, g, dskip=None):
        dw[key], du = eng.unit_backward(u, p[key], g, dskip=dskip)
        seen[key] = (u, g)
        return du

    def down(key, x, z, g, need=True):
        dw[key], dx = eng.down_backward(x, p[key], z, g, need_dx=need)
        seen[key] = (x, z, g)
        return dx

    g = dxn[2]
    for b in (2, 1):  # h -> r3 = h + U_b(U_a(h)), r4 = r3 + U_d(U_c(r3)), x = r4 + U_e(r4)
        k0, ka, kb, kc, kd, ke = CONV[4 + 6 * (b - 1):10 + 6 * (b - 1)]
        h, m3, r3, m4, r4 = units[b]
        g_r4 = unit(ke, r4, g, dskip=g)
        g_m4 = unit(kd, m4, g_r4)
        g_r3 = unit(kc, r3, g_m4, dskip=g_r4)
        g_m3 = unit(kb, m3, g_r3)
        g_h = unit(ka, h, g_m3, dskip=g_r3)
        g = dxn[b - 1] + down(k0, xs[b - 1], zs[b], g_h)  # the upsampler's dx, then the stage's
    k0, ka, kb, kc = CONV[:4]  # h -> r = h + U_b(U_a(h)), x1 = r + U_c(r)
    h, m, r = units[0]
    g_r = unit(kc, r, g, dskip=g)
    g_m = unit(kb, m, g_r)
    g_h = unit(ka, h, g_m, dskip=g_r)
    return dw, down(k0, canvas, zs[0], g_h, need=need_dx), seen
