"""-m gpu: ``gdrnpp_gt_xyz_crop`` (csrc/xyz_crop.hip) through the C ABI, the binding ``hip_lib.gt_xyz_crops``, ``gdrn_modeling.bop_xyz`` and
tools/gen_xyz.py.

Against tests/xyz_crop_ref.py the comparison is EQUALITY: coverage and depth are the oracle's fp64 expressions in the oracle's order, and
the back-projection is the same sequence of correctly rounded float32 operations in the order the kernel's header fixes (no contraction,
IEEE division, round-to-nearest-even to float16 with subnormals): the float16 bits are equal where the value is not zero, zeros compare by
value; counts, extents, boxes and offsets are integers.  Against what the reference's tool recorded (tests/golden/xyz_crop_golden.npz,
whose einsum leaves the order of the three products open) the bound is the derived one of tests/test_xyz_crop_cpu.py."""
import ctypes
import functools
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from gdrnpp_bop2022_amd import hip_lib
from gdrnpp_bop2022_amd import synthetic as S
from gdrnpp_bop2022_amd.gdrn_modeling import bop_xyz as BX
from tests import xyz_crop_golden as XG
from tests import xyz_crop_ref as XR

pytestmark = pytest.mark.gpu
DEV = "cuda"
NEAR, FAR = 0.01, 6.5
F = 203.7114                                                    # not a float32 value
NAN16 = 0x7e00


def T(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def cam(W, H):
    """A camera matrix with a skew entry, which the render and the back-projection must ignore; no entry is a float32 value."""
    return np.array([[F, 0.37, W / 2 + 0.317], [0.0, F * 1.0031, H / 2 - 0.211], [0.0, 0.0, 1.0]])


@functools.lru_cache(maxsize=None)
def models():
    """Ellipsoids of 42, 162 and 642 vertices, ~6 cm across, in metres."""
    out = []
    for sub, scale in ((1, (0.030, 0.022, 0.018)), (2, (0.030, 0.024, 0.018)), (3, (0.028, 0.028, 0.020))):
        v, f = S.icosphere(sub)
        out.append(((v * np.array(scale, np.float64)).astype(np.float32), f.astype(np.int32)))
    return out


@functools.lru_cache(maxsize=None)
def meshset():
    return hip_lib.MeshSet([v for v, _ in models()], [f for _, f in models()], DEV)


def at(K, u, v, z):
    """The translation that puts the object's centre at pixel (u, v) and depth z (metres); an irrational nudge keeps it off float32."""
    return np.array([(u - K[0, 2]) / K[0, 0] * abs(z), (v - K[1, 2]) / K[1, 1] * abs(z), z]) + np.pi * 1e-7


def pose_kinds(rng, W, H):
    """[(obj, R, t, K)]: wholly inside (one tile where the image has more), across the corner of four tiles (or the image's middle), cut by
    each image edge, wholly outside, behind the camera, crossing z_near, two instances of one object, and a refused obj."""
    K = cam(W, H)
    rot = lambda: S.random_rotation(rng)                         # noqa: E731
    cu, cv = (64.0, 64.0) if W > 64 and H > 64 else (W / 2.0, H / 2.0)
    return [(1, rot(), at(K, min(30.0, W / 2), min(31.0, H / 2), 0.5), K), (2, rot(), at(K, cu, cv, 0.5), K),
            (1, rot(), at(K, 1.5, H / 2, 0.5), K), (0, rot(), at(K, W - 1.5, H / 2, 0.5), K), (1, rot(), at(K, W / 2, 0.5, 0.5), K),
            (1, rot(), at(K, W / 2, H - 0.5, 0.5), K), (1, rot(), at(K, -150.0, H / 2, 0.5), K), (1, rot(), at(K, W / 2, H / 2, -0.5), K),
            (2, rot(), at(K, W / 2 + 9, H / 2 + 4, 0.030), K), (2, rot(), at(K, cu - 20, cv - 10, 0.55), K), (99, rot(), at(K, W / 2, H / 2, 0.5), K)]


def args_of(poses):
    return (T(np.array([p[0] for p in poses], np.int32)), T(np.stack([np.asarray(p[1], np.float64).reshape(9) for p in poses])),
            T(np.stack([np.asarray(p[2], np.float64).reshape(3) for p in poses])), T(np.stack([np.asarray(p[3], np.float64).reshape(9) for p in poses])))


def gpu(poses, W, H, ms=None, **kw):
    packed, table = hip_lib.gt_xyz_crops(ms or meshset(), *args_of(poses), (W, H), z_near=NEAR, z_far=FAR, **kw)
    assert packed.dtype == np.float16 and packed.ndim == 2 and packed.shape[1] == 3 and table.dtype == np.int64 and table.shape == (len(poses), 11)
    return packed, table


def refs_of(poses, W, H, ms=None):
    ms = ms or models()
    out = []
    for o, R, t, K in poses:
        if not 0 <= o < len(ms):
            out.append(None)
            continue
        r = XR.xyz_crop_ref(ms[o][0], ms[o][1], R, t, K, W, H, NEAR, FAR)
        r["box"] = XR.pose_box(ms[o][0], K, R, t, W, H, NEAR, FAR)
        out.append(r)
    return out


def same_f16(a, b):
    """Bit-equal where not zero, equal by value at zero."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return bool(((a.view(np.uint16) == b.view(np.uint16)) | ((a == 0) & (b == 0))).all())


def check_equal(packed, table, refs, W, H, what):
    """Every row and every element of every box against the restatement -> the pixels used."""
    off = 0
    for k, (row, r) in enumerate(zip(table.tolist(), refs)):
        if r is None:
            assert row == [-1] * 11, (what, k, row)
            continue
        b = r["box"]
        bw, bh = max(b[1] - b[0] + 1, 0), max(b[3] - b[2] + 1, 0)
        assert row[:10] == [0, r["count"]] + r["xyxy"] + b, (what, k, row, r["count"], r["xyxy"], b)
        if bw * bh == 0:
            assert r["count"] == 0
            continue
        assert row[10] == off, (what, k, row[10], off)
        if r["count"]:
            assert b[0] <= r["xyxy"][0] and r["xyxy"][2] <= b[1] and b[2] <= r["xyxy"][1] and r["xyxy"][3] <= b[3]
        got = packed[off:off + bw * bh].reshape(bh, bw, 3)
        assert same_f16(got, r["full"][b[2]:b[3] + 1, b[0]:b[1] + 1]), (what, k)
        off += bw * bh
    assert len(packed) == off, (what, len(packed), off)
    return off


# ---- 1. equality with the restatement at the tile and size edges, every pose kind ------------------------------------------------------
@pytest.mark.parametrize("W,H", [(64, 64), (65, 65), (200, 136), (1, 1)])
def test_equal_to_the_restatement(hip, W, H):
    """64x64: one exact tile; 65x65: a one-pixel last column and row of tiles; 200x136: 4x3 ragged tiles; 1x1.  Eleven poses: every kind
    of ``pose_kinds``; R, t, K are not float32 values and K has a skew entry."""
    rng = np.random.default_rng(7 + W)
    poses = pose_kinds(rng, W, H)
    for _, R, t, K in poses:
        assert not np.array_equal(R.astype(np.float32), R) and not np.array_equal(t.astype(np.float32), t) and K[0, 1] != 0
        assert not np.array_equal(K[[0, 0, 1, 1], [0, 2, 1, 2]].astype(np.float32), K[[0, 0, 1, 1], [0, 2, 1, 2]])
    refs = refs_of(poses, W, H)
    packed, table = gpu(poses, W, H)
    used = check_equal(packed, table, refs, W, H, f"{W}x{H}")
    counts = [r["count"] if r else -1 for r in refs]
    print(f"{W}x{H}: counts {counts}, boxes {[r['box'] if r else None for r in refs]}, {used} px packed")
    assert refs[6]["count"] == 0 and refs[7]["count"] == 0 and refs[7]["box"] == [1, 0, 1, 0]            # outside, behind
    assert refs[8]["box"] == [0, W - 1, 0, H - 1] and refs[8]["count"] > 0                                # crossing z_near: the whole image
    assert poses[1][0] == poses[9][0] and refs[1]["count"] > 0 and (refs[9]["count"] > 0 or W == 1) and refs[10] is None   # two instances; refused
    if (W, H) == (200, 136):
        x1, y1, x2, y2 = refs[0]["xyxy"]
        assert x2 < 64 and y2 < 64 and refs[0]["count"] > 100                                               # inside one tile
        x1, y1, x2, y2 = refs[1]["xyxy"]
        assert x1 < 64 <= x2 and y1 < 64 <= y2                                                              # across four tiles
        assert refs[2]["xyxy"][0] == 0 and refs[3]["xyxy"][2] == W - 1 and refs[4]["xyxy"][1] == 0 and refs[5]["xyxy"][3] == H - 1
    # the records of bop_xyz from this table: the true-extent slice, or the tool's invisible record
    served = [k for k, r in enumerate(refs) if r is not None]
    recs = BX.records_from_packed(packed, table[served], (W, H))
    for k, rec in zip(served, recs):
        want = XR.record(refs[k], W, H)
        assert rec["xyxy"] == want["xyxy"] and same_f16(rec["xyz_crop"], want["xyz_crop"]), k


# ---- 2. the reference's records, within the derived bound ------------------------------------------------------------------------------
def fixture_arrays():
    g = XG.load()
    poses = []
    for im, inst in g["keys"]:
        a = g["scene_gt"][im][inst]
        R, t, K = XG.tool_pose(a, g["scene_camera"][im])
        poses.append((g["obj_ids"].index(a["obj_id"]), R.astype(np.float64), t.astype(np.float64), K.astype(np.float64)))
    ms = hip_lib.MeshSet([v for v, _ in g["models_m"]], [f for _, f in g["models_m"]], DEV)
    return g, poses, ms


def test_fixture_through_the_c_abi(hip):
    g, poses, ms = fixture_arrays()
    W, H = g["im_size"]
    lib, n = hip_lib.load(), len(poses)
    a = args_of(poses)
    cap = n * H * W
    need = lib.gdrnpp_gt_xyz_crop_workspace_bytes(ms.c, n)
    assert need == n * 642 * 40 and lib.gdrnpp_gt_xyz_crop_workspace_bytes(ms.c, 0) == 0
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    out = torch.full((cap * 3,), -7.0, dtype=torch.float16, device=DEV)
    rows = torch.full((n, 12), -7, dtype=torch.int32, device=DEV)
    totals = torch.full((2,), -7, dtype=torch.int64, device=DEV)

    def call(ptrs=[x.data_ptr() for x in a], h=H, w=W, zn=g["z_near"], zf=g["z_far"], o=out.data_ptr(), c=cap, r=rows.data_ptr(), tt=totals.data_ptr(),
             nb=n, ws_ptr=ws.data_ptr(), ws_bytes=need, mc=ms.c):
        return lib.gdrnpp_gt_xyz_crop(mc, *ptrs, h, w, zn, zf, o, c, r, tt, nb, ws_ptr, ws_bytes, None)

    said = lambda text: text in lib.gdrnpp_last_error()          # noqa: E731
    p = [x.data_ptr() for x in a]
    for k in range(len(p)):
        assert call(ptrs=p[:k] + [None] + p[k + 1:]) == -1 and said(b"null pointer"), k
    assert call(o=None) == -1 and call(r=None) == -1 and call(tt=None) == -1 and said(b"null pointer")
    assert call(nb=-2) == -1 and said(b"n=-2") and call(h=0) == -1 and said(b"H=0") and call(w=-1) == -1 and said(b"W=-1")
    assert call(zn=0.0) == -1 and said(b"z_near") and call(zn=10.0, zf=5.0) == -1
    assert call(ws_bytes=need - 1) == -1 and said(b"workspace") and call(ws_ptr=None) == -1
    assert call(c=H * W - 1) == -1 and said(b"capacity") and call(mc=None) == -1 and said(b"invalid mesh set")
    assert call(nb=2 ** 30, ws_bytes=2 ** 62, c=2 ** 40) == -2 and said(b"split the poses")
    assert call(h=2 ** 20, w=2 ** 20, c=2 ** 62) == -2 and said(b"32-bit counters")
    assert call(nb=0) == 0
    torch.cuda.synchronize()
    assert (out == -7).all() and (rows == -7).all() and (totals == -7).all() and (ws == 0).all()           # nothing ran
    assert call() == 0
    torch.cuda.synchronize()
    n_done, used = totals.tolist()
    r = rows.cpu().numpy().astype(np.int64)
    assert n_done == n and (r[:, 0] == 0).all() and (r[:, 11] == 0).all()
    table = r[:, :11]
    packed = out[:3 * used].cpu().numpy().reshape(-1, 3)
    assert (out[3 * used:] == -7).all()
    worst = 0.0
    for key, rec in zip(g["keys"], BX.records_from_packed(packed, table, (W, H))):
        worst = max(worst, XG.assert_within_bound(rec, key, "C ABI"))
    print("C ABI against the reference's records: worst |ours - ref| / bound", worst)


def test_fixture_through_calc_xyz_crops(hip):
    g, _, ms = fixture_arrays()
    crops = BX.calc_xyz_crops(g["scene_gt"], g["scene_camera"], ms, g["obj_ids"], g["im_size"], g["z_near"], g["z_far"])
    assert sorted(crops) == sorted(g["keys"])
    worst = max(XG.assert_within_bound(crops[key], key, "calc_xyz_crops") for key in g["keys"])
    print("calc_xyz_crops against the reference's records: worst |ours - ref| / bound", worst)
    W, H = g["im_size"]
    for key in g["keys"]:                                       # and equal to the restatement
        want = XR.record(XG.restated()[key], W, H)
        assert crops[key]["xyxy"] == want["xyxy"] and same_f16(crops[key]["xyz_crop"], want["xyz_crop"]), key


# ---- 3. ownership of the packed buffer -----------------------------------------------------------------------------------------------------
def test_every_box_element_is_written_and_nothing_beyond(hip):
    W, H = 200, 136
    poses = pose_kinds(np.random.default_rng(31), W, H)
    cap = 4 * H * W
    out = torch.full((cap * 3,), NAN16, dtype=torch.int16, device=DEV).view(torch.float16)
    assert (out.view(torch.int16) == NAN16).all()
    packed, table = gpu(poses, W, H, out=out, capacity_px=cap)
    raw = out.view(torch.int16).cpu().numpy().view(np.uint16)
    used = 0
    for row in table.tolist():
        if row[0] != 0 or row[6] > row[7] or row[8] > row[9]:
            continue
        n_px = (row[7] - row[6] + 1) * (row[9] - row[8] + 1)
        assert row[10] == used
        assert not (raw[3 * row[10]:3 * (row[10] + n_px)] == NAN16).any(), row
        used += n_px
    assert 0 < used < cap and len(packed) == used
    assert (raw[3 * used:] == NAN16).all()
    assert np.array_equal(packed.view(np.uint16).reshape(-1), raw[:3 * used])
    check_equal(packed, table, refs_of(poses, W, H), W, H, "out=")


# ---- 4. deferral, chunking, determinism ------------------------------------------------------------------------------------------------
def count_launches(monkeypatch):
    calls = []
    real = hip_lib.pose.launch

    def counting(name, *a, **k):
        calls.append(name)
        return real(name, *a, **k)

    monkeypatch.setattr(hip_lib.pose, "launch", counting)
    return calls


def three_poses(W, H):
    rng = np.random.default_rng(5)
    K = cam(W, H)
    return [(1, S.random_rotation(rng), at(K, 40.0, 50.0, 0.5), K), (2, S.random_rotation(rng), at(K, W / 2 + 9, H / 2 + 4, 0.030), K),
            (2, S.random_rotation(rng), at(K, 130.0, 70.0, 0.45), K)]


def test_deferred_poses_are_served_by_later_launches(hip, monkeypatch):
    """capacity = one image, the middle pose crosses z_near (its box is the whole image): the first launch serves pose 0 and defers the
    other two, the second serves pose 1 alone, the third pose 2.  The binding's memory of what a pose uses is emptied first, so the second
    launch's copy is sized by the small first pose and the whole-image box takes the second copy for the rest."""
    W, H = 200, 136
    poses = three_poses(W, H)
    ample_p, ample_t = gpu(poses, W, H)
    monkeypatch.setattr(hip_lib.pose, "_XYZ_PX_PER_POSE", {})
    calls = count_launches(monkeypatch)
    packed, table = gpu(poses, W, H, capacity_px=H * W)
    assert calls == ["gdrnpp_gt_xyz_crop"] * 3
    assert table[1, 6:10].tolist() == [0, W - 1, 0, H - 1] and (table[:, 0] == 0).all()
    assert np.array_equal(table, ample_t) and np.array_equal(packed.view(np.uint16), ample_p.view(np.uint16))
    check_equal(packed, table, refs_of(poses, W, H), W, H, "deferral")
    with pytest.raises(RuntimeError, match="capacity"):
        gpu(poses, W, H, capacity_px=H * W - 1)


def test_one_pose_per_launch_equals_one_launch(hip, monkeypatch):
    W, H = 200, 136
    poses = pose_kinds(np.random.default_rng(11), W, H)
    one_p, one_t = gpu(poses, W, H)
    per_pose = hip_lib.load().gdrnpp_gt_xyz_crop_workspace_bytes(meshset().c, 1)
    calls = count_launches(monkeypatch)
    packed, table = gpu(poses, W, H, workspace_budget=per_pose)
    assert len(calls) == len(poses)
    assert np.array_equal(table, one_t) and np.array_equal(packed.view(np.uint16), one_p.view(np.uint16))


def test_two_calls_are_bit_equal(hip):
    W, H = 200, 136
    poses = pose_kinds(np.random.default_rng(13), W, H)
    a, b = gpu(poses, W, H), gpu(poses, W, H)
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[0].view(np.uint16), b[0].view(np.uint16))
    e_p, e_t = hip_lib.gt_xyz_crops(meshset(), *[x[:0] for x in args_of(poses)], (W, H))
    assert e_p.shape == (0, 3) and e_t.shape == (0, 11)
    with pytest.raises(RuntimeError, match="dtype"):
        x = args_of(poses)
        hip_lib.gt_xyz_crops(meshset(), x[0], x[1].float(), x[2], x[3], (W, H))


# ---- 5. the command-line tool end to end ---------------------------------------------------------------------------------------------------
def test_gen_xyz_writes_the_split(hip, tmp_path):
    g, _, ms = fixture_arrays()
    W, H = g["im_size"]
    d, split, scene = XG.write_split(tmp_path)
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_xyz.py"), "--dataset-dir", d, "--split", split, "--models-dir", "models",
                          "--im-size", str(W), str(H)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.count("not visible, cls") == 2 and f"scene {scene:06d}: 3 images, 12 instances, 12 files written, 2 not visible" in run.stdout
    crops = BX.calc_xyz_crops(g["scene_gt"], g["scene_camera"], ms, g["obj_ids"], (W, H), g["z_near"], g["z_far"])
    for (im, inst), want in crops.items():
        with open(os.path.join(d, split, "xyz_crop", f"{scene:06d}", f"{im:06d}_{inst:06d}-xyz.pkl"), "rb") as f:
            got = pickle.load(f)
        assert got["xyxy"] == want["xyxy"] and got["xyz_crop"].dtype == np.float16
        assert np.array_equal(got["xyz_crop"].view(np.uint16), want["xyz_crop"].view(np.uint16)), (im, inst)
        XG.assert_within_bound(got, (im, inst), "gen_xyz.py")
