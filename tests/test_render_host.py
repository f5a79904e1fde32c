"""CPU: the MJCF loader (robot_aware_control_amd/mjcf.py), the fp64 restatement of the mask renderer the GPU tests compare
with (tests/render_refs.py) and the host-side wiring of `--robot_mjcf`.

The restatement is checked on its own ground first: forward kinematics against closed forms, the camera convention
against an OpenCV pinhole projection, and the width of its undecidable band hi ^ lo -- at most 1 % of an image for every
pose a GPU test uses -- before any GPU mask is compared with it."""
import argparse
import os
import re

import numpy as np
import pytest
import torch

from tests import render_refs as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAND_CAP = 0.01


# ---- loader ------------------------------------------------------------------------------------------------------------

def _expected_triangles(path):
    """Sum of the STL headers' counts over the mesh geoms + 12 per box, read with nothing but ElementTree and struct."""
    import xml.etree.ElementTree as ET
    root = ET.parse(path).getroot()
    meshdir = os.path.join(os.path.dirname(path), root.find("compiler").get("meshdir"))
    files = {m.get("name"): os.path.join(meshdir, m.get("file")) for m in root.find("asset").findall("mesh")}
    n = 0
    for g in root.find("worldbody").iter("geom"):
        n += rr.stl_count(files[g.get("mesh")]) if g.get("type") == "mesh" else 12
    return n


def test_loader_tables_wx250s():
    from robot_aware_control_amd import mjcf
    m = mjcf.load_mjcf(rr.WX250S)
    assert m.name == "wx250s" and m.native_hw == (48, 64) and m.joints == tuple(rr.WX250S_JOINTS)
    assert m.link_names == ["world"] + ["wx250s/" + n for n in (
        "shoulder_link", "upper_arm_link", "upper_forearm_link", "lower_forearm_link", "wrist_link", "gripper_link",
        "gripper_prop_link", "left_finger_link", "right_finger_link")]
    assert m.link_parent.tolist() == [-1, 0, 1, 2, 3, 4, 5, 6, 6, 6]
    assert m.joint_names == [None, "waist", "shoulder", "elbow", "forearm_roll", "wrist_angle", "wrist_rotate", "gripper",
                             "left_finger", "right_finger"]
    assert m.joint_type.tolist() == [0, 1, 1, 1, 1, 1, 1, 1, 2, 2]
    assert m.joint_col.tolist() == [-1, 0, 1, 2, 3, 4, 5, -1, -1, -1]      # unlisted joints stay at 0
    assert m.joint_axis[1].tolist() == [0, 0, 1] and m.joint_axis[4].tolist() == [1, 0, 0]
    assert np.allclose(m.link_pos[3], [0.04975, 0, 0.25]) and np.allclose(np.linalg.norm(m.link_quat, axis=1), 1)
    cam = m.cameras["main_cam"]
    assert cam.link == 0 and cam.fovy == 43.3 and np.allclose(cam.pos, [0.81822263, -0.05511966, 0.45810006])
    assert np.isclose(np.linalg.norm(cam.quat), 1)
    assert len(m.tri) == _expected_triangles(rr.WX250S) == 12460 and m.tri.dtype == np.float32
    assert m.tri_robot.all() and len(m.tri_link) == len(m.tri_robot) == len(m.tri)
    assert [m.link_depth(l) for l in range(m.n_links)] == [0, 1, 2, 3, 4, 5, 6, 7, 7, 7]


def test_loader_tables_widowx():
    from robot_aware_control_amd import mjcf
    m = mjcf.load_mjcf(rr.WIDOWX)
    assert m.name == "widowx_arm" and m.native_hw == (64, 85) and m.joints == tuple(rr.WIDOWX_JOINTS)
    assert m.link_names == ["world", "base", "eef_body", "shoulder_link", "biceps_link", "forearm_link", "wrist_1_link",
                            "wrist_2_link", "gripper_aux_link"]
    assert m.link_parent.tolist() == [-1, 0, 1, 1, 3, 4, 5, 6, 7]
    assert m.joint_col.tolist() == [-1, -1, -1, 0, 1, 2, 3, 4, 5]
    assert np.allclose(m.link_quat[5], np.array([0.707107, 0, 0.707106, 0]) / np.linalg.norm([0.707107, 0.707106]))
    assert m.cameras["main_cam"].link == 1                                   # the camera hangs on the `base` body
    assert len(m.tri) == _expected_triangles(rr.WIDOWX) == 3220
    # the unnamed 12-triangle box is the one geom that is not robot; base_link_mesh is ("mesh" in its name)
    assert m.geom_names[0] is None and m.geom_tris[0] == 12 and int((~m.tri_robot).sum()) == 12
    assert m.geom_names[1] == "base_link_mesh" and m.tri_robot[12:].all()
    for name, want in (("base_link_vis", False), ("head_vis", False), (None, False), ("table", False),
                       ("arm_col", True), ("gripper_1", True)):
        assert mjcf.NAMED["widowx_arm"][1](name) is want, name


def test_loader_matches_the_restatements_reader():
    """Two readers written separately give the same link-local mesh triangles, links and robot flags."""
    from robot_aware_control_amd import mjcf
    for path, joints, rule in ((rr.WX250S, rr.WX250S_JOINTS, lambda n: True), (rr.WIDOWX, rr.WIDOWX_JOINTS,
                                                                                  rr.widowx_is_robot)):
        m, ref = mjcf.load_mjcf(path), rr.read_model(path, joints, rule)
        assert np.array_equal(ref["tri_link"], m.tri_link) and np.array_equal(ref["tri_robot"], m.tri_robot)
        mesh = ref["tri_robot"] | (m.tri_link > 1)
        assert np.allclose(ref["tris"][mesh], m.tri[mesh], rtol=0, atol=1e-7)
        for l, (name, parent, X, joint) in enumerate(ref["links"]):
            assert parent == m.link_parent[l] and np.allclose(X[:3, :3], mjcf.quat_to_mat(m.link_quat[l]))


BODY = '<body name="b" pos="0 0 1"><joint name="j"/><geom type="box" size="1 1 1"/>{}</body>'
UNSUPPORTED = [
    ("include", '<include file="other.xml"/>', ""),
    ("default", '<default><geom rgba="1 0 0 1"/></default>', ""),
    ("euler", "", '<body euler="0 0 1.57"><geom type="sphere" size="1"/></body>'),
    ("axisangle", "", '<geom type="sphere" size="1" axisangle="0 0 1 1"/>'),
    ("xyaxes", "", '<camera name="c" xyaxes="1 0 0 0 1 0"/>'),
    ("zaxis", "", '<geom type="sphere" size="1" zaxis="0 1 0"/>'),
    ("fromto", "", '<geom type="capsule" size="0.1" fromto="0 0 0 0 0 1"/>'),
    ("ellipsoid", "", '<geom type="ellipsoid" size="1 2 3"/>'),
    ("plane", "", '<geom type="plane" size="1 1 1"/>'),
    ("hfield", "", '<geom type="hfield" hfield="h"/>'),
    ("ref", "", '<body><joint name="k" ref="0.3"/><geom type="sphere" size="1"/></body>'),
    ("ball", "", '<body><joint name="k" type="ball"/><geom type="sphere" size="1"/></body>'),
    ("more than one joint", "", '<body><joint name="k"/><joint name="l"/><geom type="sphere" size="1"/></body>'),
]


@pytest.mark.parametrize("what,top,inner", UNSUPPORTED, ids=[u[0] for u in UNSUPPORTED])
def test_loader_refuses_what_it_does_not_read(tmp_path, what, top, inner):
    from robot_aware_control_amd import mjcf
    path = tmp_path / "m.xml"
    path.write_text(f'<mujoco model="t"><compiler angle="radian"/>{top}<worldbody>{BODY.format(inner)}</worldbody></mujoco>')
    with pytest.raises(ValueError, match=what):
        mjcf.load_mjcf(str(path), joints=["j"], is_robot_geom=lambda n: True)


def test_loader_degrees_with_a_rotation_and_unknown_models(tmp_path):
    from robot_aware_control_amd import mjcf
    path = tmp_path / "m.xml"
    path.write_text('<mujoco model="t"><compiler angle="degree"/><worldbody><body euler="0 0 90">'
                    '<geom type="sphere" size="1"/></body></worldbody></mujoco>')
    with pytest.raises(ValueError, match="degrees"):
        mjcf.load_mjcf(str(path), joints=[], is_robot_geom=lambda n: True)
    path.write_text('<mujoco model="t"><worldbody>' + BODY.format("") + "</worldbody></mujoco>")
    with pytest.raises(ValueError, match="joints="):                 # an unknown model brings no joint list
        mjcf.load_mjcf(str(path))
    with pytest.raises(ValueError, match="defined 0 times"):
        mjcf.load_mjcf(str(path), joints=["nope"], is_robot_geom=lambda n: True)
    m = mjcf.load_mjcf(str(path), joints=["j"], is_robot_geom=lambda n: n == "x")
    assert m.joint_col.tolist() == [-1, 0] and len(m.tri) == 12 and not m.tri_robot.any()


def test_primitives_and_stl(tmp_path):
    from robot_aware_control_amd import mjcf
    assert mjcf.SEGMENTS >= 16
    box = mjcf.primitive("box", [1, 2, 3])
    assert box.shape == (12, 3, 3) and np.abs(box).max(axis=(0, 1)).tolist() == [1, 2, 3]
    n = np.cross(box[:, 1] - box[:, 0], box[:, 2] - box[:, 0])
    assert np.isclose(0.5 * np.linalg.norm(n, axis=1).sum(), 2 * (2 * 4 + 2 * 6 + 4 * 6))       # the box's surface
    sph = mjcf.primitive("sphere", [0.5])
    assert sph.shape == (224, 3, 3) and np.allclose(np.linalg.norm(sph, axis=2), 0.5)
    cyl = mjcf.primitive("cylinder", [0.5, 2.0])
    assert cyl.shape == (64, 3, 3) and np.abs(cyl[..., 2]).max() == 2.0
    rim = cyl.reshape(-1, 3)
    assert np.allclose(np.linalg.norm(rim[np.linalg.norm(rim[:, :2], axis=1) > 0][:, :2], axis=1), 0.5)
    cap = mjcf.primitive("capsule", [0.5, 2.0]).reshape(-1, 3)
    assert len(cap) == 256 * 3 and np.isclose(np.abs(cap[:, 2]).max(), 2.5)
    axis_dist = np.linalg.norm(cap - np.clip(cap * [0, 0, 1], -2.0, 2.0), axis=1)                # to the segment
    assert np.allclose(axis_dist, 0.5)
    for tris in (sph, cyl, mjcf.primitive("capsule", [0.5, 2.0])):                               # no zero-area triangle
        assert (np.linalg.norm(np.cross(tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]), axis=1) > 1e-9).all()
    # STL: the length decides, a leading `solid` does not
    tri = np.arange(18, dtype=np.float32).reshape(2, 3, 3)
    rr.write_stl(str(tmp_path / "a.stl"), tri)
    assert open(tmp_path / "a.stl", "rb").read(5) == b"solid" and np.array_equal(mjcf.read_stl(str(tmp_path / "a.stl")), tri)
    with open(tmp_path / "a.stl", "ab") as f:
        f.write(b"\0")
    with pytest.raises(ValueError, match="2 triangles"):
        mjcf.read_stl(str(tmp_path / "a.stl"))
    assert open(os.path.join(rr.GOLDEN, "stls", "widowx", "base_link.stl"), "rb").read(5) == b"solid"


def test_opencv_camera_pose_is_the_reference_call():
    """pos = ext[:3, 3] + offset, rotation = R(ext) Ry(180 deg) (base_mask_env.py:8-22), and the quaternion round trip."""
    from robot_aware_control_amd import mjcf
    rs = np.random.RandomState(3)
    for _ in range(20):
        q = rs.randn(4)
        ext = rr.pose(rs.randn(3), rr.rot(q))
        pos, quat = mjcf.opencv_camera_pose(ext, offset=(0.1, 0.2, 0.3))
        want = rr.opencv_camera(ext, (0.1, 0.2, 0.3))
        assert np.allclose(pos, want[:3, 3]) and np.allclose(mjcf.quat_to_mat(quat), want[:3, :3], atol=1e-12)
    for path in (rr.WX250S, rr.WIDOWX):      # the loader's and the restatement's cameras agree
        m = mjcf.load_mjcf(path)
        cam = m.cameras["main_cam"]
        ref = rr.read_model(path, [])["cams"]["main_cam"]
        assert cam.link == ref[0] and np.allclose(mjcf.quat_to_mat(cam.quat), ref[1][:3, :3]) and cam.fovy == ref[2]


# ---- the restatement on its own ground -----------------------------------------------------------------------------------

def test_restatement_forward_kinematics_closed_form():
    model = rr.read_model(rr.WX250S, rr.WX250S_JOINTS)
    grip = [l[0] for l in model["links"]].index("wx250s/gripper_link")
    assert np.allclose(rr.forward_kinematics(model, np.zeros(6))[grip, :3, 3], [0.36475, 0, 0.36065], atol=1e-12)
    q = np.zeros(6)
    q[0] = np.pi / 2
    assert np.allclose(rr.forward_kinematics(model, q)[grip, :3, 3], [0, 0.36475, 0.36065], atol=1e-12)
    # shoulder = pi/2 lays the arm forward: the upper arm's (0.04975, 0, 0.25) offset turns about y
    q = np.zeros(6)
    q[1] = np.pi / 2
    fore = [l[0] for l in model["links"]].index("wx250s/upper_forearm_link")
    assert np.allclose(rr.forward_kinematics(model, q)[fore, :3, 3], [0.25, 0, 0.072 + 0.03865 - 0.04975], atol=1e-12)


def _speck(point, ext, size):
    """A model that is one small robot triangle around a world point, facing the camera of `ext`."""
    R = np.asarray(ext)[:3, :3]
    tri = np.array([point + size * (R[:, 0] * a + R[:, 1] * b) for a, b in ((-1, -1), (1, -1), (0, 1.5))])
    return dict(links=[("world", -1, np.eye(4), None)], tris=tri[None], tri_link=np.zeros(1, int),
                tri_robot=np.ones(1, bool), cams={"main_cam": (0, np.eye(4), 50.0)}, joints=[])


def test_restatement_camera_convention():
    """After set_opencv_camera_pose(ext) the image is the OpenCV pinhole image of camera-to-world ext: a point on the
    optical axis lands on the centre pixel, one toward +x to its right, one toward +y below it -- and exactly where
    fx = fy = f, cx = W/2, cy = H/2 put it."""
    H, W = 11, 15
    rs = np.random.RandomState(5)
    ext = rr.pose(np.array([0.3, -0.2, 0.5]), rr.rot(rs.randn(4)))
    R, p = ext[:3, :3], ext[:3, 3]
    f = 0.5 * H / np.tan(np.radians(50.0) / 2)
    cam = rr.opencv_camera(ext)
    for dx, dy in ((0, 0), (3, 0), (0, 2), (-4, -3)):
        point = p + R @ np.array([dx / f, dy / f, 1.0]) * 0.8      # dx pixels right, dy pixels down at depth 0.8
        lo, mid, hi = rr.render(_speck(point, ext, 0.3 * 0.8 / f), np.zeros(0), cam, H=H, W=W)
        rows, cols = np.nonzero(mid)
        assert rows.tolist() == [H // 2 + dy] and cols.tolist() == [W // 2 + dx], (dx, dy, rows, cols)
        x, y = rr.pinhole(ext, point, 50.0, H, W)
        assert np.isclose(x, W / 2 + dx) and np.isclose(y, H / 2 + dy)
    # the same camera WITHOUT the call looks the other way: nothing is seen
    lo, mid, hi = rr.render(_speck(p + R[:, 2] * 0.8, ext, 0.01), np.zeros(0), ext, H=H, W=W)
    assert not hi.any()


@pytest.mark.parametrize("which", ["wx250s", "widowx"])
def test_band_cap_fixtures(which):
    model, cam, H, W, qs, results = rr.fixture_case(which)
    assert len(qs) == 3
    for q, (lo, mid, hi) in zip(qs, results):
        assert not (lo & ~mid).any() and not (mid & ~hi).any()
        assert 100 <= mid.sum() <= 300, mid.sum()
        assert rr.band_fraction(lo, hi) <= BAND_CAP, rr.band_fraction(lo, hi)
    # the XML's camera pose is stored OpenCV-style: rendered without set_opencv_camera_pose the robot is behind it
    assert not rr.render(model, qs[0], model["cams"]["main_cam"][1], H=H, W=W)[2].any()


def test_band_cap_hand_made(tmp_path):
    model = rr.read_model(rr.write_hand_model(str(tmp_path)), rr.HAND_JOINTS, rr.hand_is_robot)
    cam = rr.opencv_camera(rr.HAND_EXT)
    for (H, W), poses in (((12, 16), rr.HAND_POSES), ((128, 128), rr.HAND_POSES[1:2])):
        for q in poses:
            lo, mid, hi = rr.render(model, q, cam, H=H, W=W)
            assert mid.any() and rr.band_fraction(lo, hi) <= BAND_CAP
            # the non-robot box hides robot pixels: the same scene with every geom robot shows more
            every = rr.render(dict(model, tri_robot=np.ones_like(model["tri_robot"])), q, cam, H=H, W=W)[1]
            assert (every & ~mid).sum() >= 10 * (H // 12)
    # the plate crosses the right and the bottom border, one triangle has a vertex behind znear, one has no area
    u, v, d, _ = rr.project(model, rr.HAND_POSES[0], cam, H=12, W=16)
    robot = np.nonzero(model["tri_robot"])[0]
    plate, near, flat = robot[0], robot[1], robot[2]
    assert (16 - u[plate]).max() > 16 and (12 - v[plate]).max() > 11.5 and (d[near] < rr.ZNEAR).any()
    area = (u[:, 1] - u[:, 0]) * (v[:, 2] - v[:, 0]) - (v[:, 1] - v[:, 0]) * (u[:, 2] - u[:, 0])
    assert area[flat] == 0 and (d[plate] > rr.ZNEAR).all()


# ---- the ABI and the wiring ------------------------------------------------------------------------------------------------

def test_header_declares_the_entry_and_keeps_the_abi_version():
    hdr = open(os.path.join(ROOT, "include", "rac_hip.h")).read()
    assert "int rac_render_masks(" in hdr and "#define RAC_ABI_VERSION 12" in hdr
    assert re.search(r"#define RAC_RENDER_MAX_PIXELS 16384\b", hdr)
    from robot_aware_control_amd import EXPORTS, _lib
    assert "rac_render_masks" in EXPORTS and len(_lib._SIGS["rac_render_masks"]) == 22 and _lib.ABI_VERSION == 12
    assert _lib.load().rac_render_link_bytes() == 88


def test_renderer_is_gpu_only_and_checks_its_arguments():
    from robot_aware_control_amd import RacError
    from robot_aware_control_amd.render import MjcfMaskRenderer
    r = MjcfMaskRenderer(rr.WX250S)
    assert (r._img_height, r._img_width, r._camera_name) == (48, 64, "main_cam") and len(r.joints) == 6
    with pytest.raises(RacError, match="GPU only"):
        r.render(torch.zeros(2, 6))
    with pytest.raises(ValueError, match="no camera"):
        MjcfMaskRenderer(rr.WX250S, camera="side_cam")
    with pytest.raises(ValueError, match="no camera"):
        r.set_opencv_camera_pose("side_cam", np.eye(4))
    with pytest.raises(ValueError, match=r"\(4, 4\)"):
        r.set_opencv_camera_pose("main_cam", np.eye(3))


def test_flags_and_mask_renderer_route(tmp_path):
    from robot_aware_control_amd import config as rcfg
    from robot_aware_control_amd.heatmaps import CameraTable
    from robot_aware_control_amd.render import MjcfMaskRenderer
    from robot_aware_control_amd.robot_model import mask_renderer
    cf = rcfg.create_parser("FetchPush").parse_args([])
    assert cf.robot_mjcf is None and cf.robot_mjcf_camera == "main_cam"
    cf = rcfg.create_parser("FetchPush").parse_args(["--robot_mjcf", rr.WIDOWX, "--robot_mjcf_camera", "main_cam"])
    assert cf.robot_mjcf == rr.WIDOWX
    ext = rr.pose(np.array([1.0, 0.2, 0.4]), rr.rot([0.3, -0.5, 0.6, 0.2]))
    table = CameraTable({"widowx_cam3": np.linalg.inv(ext)}, {})
    table.save(str(tmp_path / "cal.npz"))
    ns = argparse.Namespace(experiment="finetune_widowx", robot_mjcf=rr.WIDOWX, robot_mjcf_camera="main_cam",
                            camera_calibration=str(tmp_path / "cal.npz"))
    renderers = {}
    env = mask_renderer(renderers, ns, "cam3")
    assert isinstance(env, MjcfMaskRenderer) and renderers["cam3"] is env and mask_renderer(renderers, ns, "cam3") is env
    pos, quat = env._poses["main_cam"]
    want = rr.opencv_camera(ext)
    from robot_aware_control_amd import mjcf
    assert np.allclose(pos, want[:3, 3]) and np.allclose(mjcf.quat_to_mat(quat), want[:3, :3])
    with pytest.raises(NotImplementedError, match="widowx_cam9"):
        mask_renderer({}, ns, "cam9")
    # without --robot_mjcf the route is the reference environments', as before
    ns.robot_mjcf = None
    with pytest.raises(NotImplementedError, match="reference checkout"):
        mask_renderer({}, ns, "cam3")
