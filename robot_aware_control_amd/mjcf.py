"""A reader for the subset of MuJoCo's MJCF that the robot-mask renderer needs (host side, numpy only).

`load_mjcf(path)` turns a robot description into the flat tables `rac_render_masks` consumes (render.py):

* links, parents first: parent, local pose (`pos`, `quat` w x y z, normalised on read) and at most one joint (hinge or
  slide: axis, anchor, the column of a qpos row that drives it; a joint nobody drives stays at 0);
* triangles in LINK-LOCAL coordinates with the geom's own `pos` / `quat` applied, each with its link and a robot flag:
  binary STL meshes (`file coords * scale`) and the primitives, tessellated here;
* cameras: parent link, local pose, `fovy` in degrees.

What is read: `<compiler angle meshdir>`, `<asset><mesh name file scale>`, and under `<worldbody>` the tree of
`<body pos quat>`, `<joint name type axis pos>`, `<geom name type mesh size pos quat>`, `<camera name fovy pos quat>`.
`inertial`, `site`, `light`, textures, materials, `rgba`, `contype`, `conaffinity`, `group`, masses, limits and the
like do not move a triangle and are skipped.  Everything that WOULD move one and is not in the subset raises a
ValueError that names it: `<include>`, `<default>`, `euler`, `axisangle`, `xyaxes`, `zaxis`, `fromto`, a `ref` on a
joint, ball / free joints, two joints on one body, ellipsoid / plane / hfield geoms, mesh `refpos` / `refquat`, tracking
cameras.  Nothing here looks at `angle="degree"` except to say so in the message when a rotation attribute is refused:
quaternions have no unit, `fovy` is always degrees and a hinge's qpos always radians.

Tessellation of the primitives (fixed, so that a model's triangle table is reproducible): a box is 12 triangles; the
round ones are surfaces of revolution about the geom's z axis with SEGMENTS = 16 sides -- a sphere has 8 latitude bands
(224 triangles), a cylinder a side and two fans (64), a capsule a side and two 4-band hemispheres (256).  The vertices
lie ON the surface, so the silhouette is inscribed: at most r (1 - cos(pi / 16)) = 1.9 % of the radius inside the true one.
"""
from __future__ import annotations

import os
import xml.etree.ElementTree as ET
from dataclasses import dataclass, field

import numpy as np

SEGMENTS = 16      # sides of a round primitive
BANDS = 8          # latitude bands of a sphere (4 per capsule hemisphere)
MAX_LINKS = 64     # RAC_RENDER_MAX_LINKS
JOINT_NONE, JOINT_HINGE, JOINT_SLIDE = 0, 1, 2

_ORIENT = ("euler", "axisangle", "xyaxes", "zaxis", "fromto")
_TOP_IGNORED = {"compiler", "size", "option", "visual", "statistic", "asset", "worldbody", "actuator", "sensor",
                "contact", "equality", "tendon", "keyframe", "custom"}
_ASSET_IGNORED = {"texture", "material", "skin"}
_BODY_IGNORED = {"inertial", "site", "light"}

_WIDOWX_NOT_ROBOT = ("base_link_vis", "base_link_col", "head_vis")


def _widowx_is_robot(name):
    return (name is not None and name not in _WIDOWX_NOT_ROBOT
            and any(part in name for part in ("vis", "col", "gripper", "mesh")))


# model= name -> (driven joints in qpos order, is_robot_geom(name or None), native (height, width)): the reference mask
# environments' lists (wx250s_mask_env.py:22-25,76-79; widowx_mask_env.py:20-24,66-77)
NAMED = {
    "wx250s": (("waist", "shoulder", "elbow", "forearm_roll", "wrist_angle", "wrist_rotate"), lambda name: True, (48, 64)),
    "widowx_arm": (("joint_1", "joint_2", "joint_3", "joint_4", "joint_5", "gripper_revolute_joint"), _widowx_is_robot,
                   (64, 85)),
}


@dataclass
class MjcfCamera:
    name: str
    link: int
    pos: np.ndarray    # (3,) in the link's frame
    quat: np.ndarray   # (4,) w x y z: MuJoCo's camera frame (looks along -z, +x right, +y up)
    fovy: float        # degrees


@dataclass
class MjcfModel:
    name: str
    link_names: list
    link_parent: np.ndarray    # (L,) int32, -1 for the world (link 0); parents come first
    link_pos: np.ndarray       # (L, 3) float64
    link_quat: np.ndarray      # (L, 4) float64, w x y z, unit
    joint_names: list          # per link: the joint's name or None
    joint_type: np.ndarray     # (L,) int32: JOINT_NONE / JOINT_HINGE / JOINT_SLIDE
    joint_axis: np.ndarray     # (L, 3) float64, unit, in the link's frame
    joint_anchor: np.ndarray   # (L, 3) float64, in the link's frame
    joint_col: np.ndarray      # (L,) int32: the qpos column that drives the link's joint, -1: stays at 0
    joints: tuple              # the driven joints' names, qpos order
    tri: np.ndarray            # (N, 3, 3) float32: triangle, vertex, xyz -- link-local
    tri_link: np.ndarray       # (N,) int32
    tri_robot: np.ndarray      # (N,) bool
    geom_names: list           # per geom, None where unnamed
    geom_tris: list            # per geom: its triangle count
    cameras: dict = field(default_factory=dict)
    native_hw: tuple = (48, 64)

    @property
    def n_links(self):
        return len(self.link_names)

    def link_depth(self, link: int) -> int:
        """Links on the chain from the world to `link`, itself included (the world is 0)."""
        d = 0
        while self.link_parent[link] >= 0:
            link, d = int(self.link_parent[link]), d + 1
        return d


def quat_to_mat(q) -> np.ndarray:
    w, x, y, z = np.asarray(q, dtype=np.float64)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def mat_to_quat(R) -> np.ndarray:
    """w x y z of a rotation matrix (the largest component first, for conditioning)."""
    R = np.asarray(R, dtype=np.float64)
    K = np.array([R[0, 0] + R[1, 1] + R[2, 2], R[0, 0] - R[1, 1] - R[2, 2], R[1, 1] - R[0, 0] - R[2, 2],
                  R[2, 2] - R[0, 0] - R[1, 1]])
    i = int(np.argmax(K))
    s = np.sqrt(1.0 + K[i]) * 2
    if i == 0:
        q = [0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s]
    elif i == 1:
        q = [(R[2, 1] - R[1, 2]) / s, 0.25 * s, (R[0, 1] + R[1, 0]) / s, (R[0, 2] + R[2, 0]) / s]
    elif i == 2:
        q = [(R[0, 2] - R[2, 0]) / s, (R[0, 1] + R[1, 0]) / s, 0.25 * s, (R[1, 2] + R[2, 1]) / s]
    else:
        q = [(R[1, 0] - R[0, 1]) / s, (R[0, 2] + R[2, 0]) / s, (R[1, 2] + R[2, 1]) / s, 0.25 * s]
    q = np.array(q)
    return q / np.linalg.norm(q)


def read_stl(path) -> np.ndarray:
    """(n, 3, 3) float32 vertices of a BINARY STL: 80-byte header, uint32 count, 50 bytes per triangle.  The length
    decides, not a leading `solid` (binary exports that start with it exist)."""
    with open(path, "rb") as f:
        raw = f.read()
    if len(raw) < 84:
        raise ValueError(f"{path}: {len(raw)} bytes is no binary STL")
    n = int(np.frombuffer(raw, "<u4", 1, 80)[0])
    if len(raw) != 84 + 50 * n:
        raise ValueError(f"{path}: header says {n} triangles = {84 + 50 * n} bytes, the file has {len(raw)} "
                         f"(ASCII STL is not read)")
    rec = np.frombuffer(raw, np.dtype([("n", "<f4", 3), ("v", "<f4", (3, 3)), ("a", "<u2")]), n, 84)
    return np.array(rec["v"], dtype=np.float32)


def _box(size):
    hx, hy, hz = size
    v = np.array([[sx * hx, sy * hy, sz * hz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], dtype=np.float64)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    return np.array([[v[a], v[b], v[c]] for q in quads for a, b, c in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))])


def _revolve(profile):
    """The surface of revolution of a (radius, z) polyline about z with SEGMENTS sides; radius 0 is a pole."""
    ang = 2 * np.pi * np.arange(SEGMENTS + 1) / SEGMENTS
    c, s = np.cos(ang), np.sin(ang)
    c[-1], s[-1] = c[0], s[0]
    tris = []
    for (r0, z0), (r1, z1) in zip(profile[:-1], profile[1:]):
        for i in range(SEGMENTS):
            a0, a1 = [r0 * c[i], r0 * s[i], z0], [r0 * c[i + 1], r0 * s[i + 1], z0]
            b0, b1 = [r1 * c[i], r1 * s[i], z1], [r1 * c[i + 1], r1 * s[i + 1], z1]
            if r0 != 0:
                tris.append([a0, a1, b1])
            if r1 != 0:
                tris.append([a0, b1, b0])
    return np.array(tris, dtype=np.float64)


def _arc(r, z, lo, hi, n):
    """n bands of a circle of radius r centred on (0, z), polar angle lo..hi measured from -z; exact poles."""
    th = np.linspace(lo, hi, n + 1)
    rr, zz = r * np.sin(th), z - r * np.cos(th)
    rr[np.isclose(rr, 0, atol=1e-15 * max(r, 1))] = 0.0
    return list(zip(rr, zz))


def primitive(gtype: str, size) -> np.ndarray:
    """(n, 3, 3) float64 triangles of a primitive geom in its own frame (the module docstring has the tessellation)."""
    size = [float(x) for x in size]
    need = {"box": 3, "sphere": 1, "cylinder": 2, "capsule": 2}[gtype]
    if len(size) < need:
        raise ValueError(f"geom type {gtype!r} needs size with {need} numbers, got {size} (fromto is not read)")
    if gtype == "box":
        return _box(size[:3])
    r = size[0]
    if gtype == "sphere":
        return _revolve(_arc(r, 0.0, 0.0, np.pi, BANDS))
    hh = size[1]
    if gtype == "cylinder":
        return _revolve([(0.0, -hh), (r, -hh), (r, hh), (0.0, hh)])
    return _revolve(_arc(r, -hh, 0.0, np.pi / 2, BANDS // 2) + _arc(r, hh, np.pi / 2, np.pi, BANDS // 2))


def _floats(el, attr, default, n=None):
    s = el.get(attr)
    if s is None:
        return np.array(default, dtype=np.float64)
    v = np.array([float(x) for x in s.split()], dtype=np.float64)
    if n is not None and len(v) != n:
        raise ValueError(f"<{el.tag} {attr}={s!r}>: {n} numbers expected")
    return v


def _quat(el):
    q = _floats(el, "quat", (1, 0, 0, 0), 4)
    n = np.linalg.norm(q)
    if n == 0:
        raise ValueError(f"<{el.tag} quat> is zero")
    return q / n


def load_mjcf(path, joints=None, is_robot_geom=None, native_hw=None) -> MjcfModel:
    """Read `path`.  The models of NAMED bring their driven joints, robot-geom rule and native render size; any other
    model takes `joints` (names, qpos order) and `is_robot_geom(name_or_None) -> bool` from the caller, who may also
    override them for a named one."""
    path = os.fspath(path)
    root = ET.parse(path).getroot()
    if root.tag != "mujoco":
        raise ValueError(f"{path}: root element <{root.tag}>, not <mujoco>")
    name = root.get("model", "")
    for el in root.iter():
        if el.tag in ("include", "default"):
            raise ValueError(f"{path}: <{el.tag}> is not read (flatten the model first)")
    for el in root:
        if el.tag not in _TOP_IGNORED:
            raise ValueError(f"{path}: top-level <{el.tag}> is not read")
    known = NAMED.get(name)
    if joints is None:
        if known is None:
            raise ValueError(f"{path}: model {name!r} is not one of {sorted(NAMED)}: pass joints= and is_robot_geom=")
        joints = known[0]
    if is_robot_geom is None:
        if known is None:
            raise ValueError(f"{path}: model {name!r} is not one of {sorted(NAMED)}: pass is_robot_geom=")
        is_robot_geom = known[1]
    if native_hw is None:
        native_hw = known[2] if known else (48, 64)
    joints = tuple(joints)

    angle, meshdir = "degree", ""
    for comp in root.findall("compiler"):
        angle = comp.get("angle", angle)
        meshdir = comp.get("meshdir", meshdir)
        if comp.get("coordinate", "local") != "local":
            raise ValueError(f"{path}: <compiler coordinate={comp.get('coordinate')!r}> is not read")

    def refuse_orientation(el):
        for a in _ORIENT:
            if el.get(a) is not None:
                unit = " (and the file's angles are in degrees)" if angle == "degree" and a in ("euler", "axisangle") else ""
                raise ValueError(f"{path}: <{el.tag} {a}=...> is not read: give pos / quat{unit}")

    meshes = {}
    base = os.path.join(os.path.dirname(path), meshdir)
    for asset in root.findall("asset"):
        for el in asset:
            if el.tag == "mesh":
                for a in ("refpos", "refquat", "vertex"):
                    if el.get(a) is not None:
                        raise ValueError(f"{path}: <mesh {a}=...> is not read")
                file = el.get("file")
                if file is None:
                    raise ValueError(f"{path}: <mesh> without file=")
                mname = el.get("name") or os.path.splitext(os.path.basename(file))[0]
                meshes[mname] = (os.path.join(base, file), _floats(el, "scale", (1, 1, 1), 3))
            elif el.tag == "hfield":
                raise ValueError(f"{path}: <hfield> is not read")
            elif el.tag not in _ASSET_IGNORED:
                raise ValueError(f"{path}: <asset><{el.tag}> is not read")

    stl_cache = {}
    links = dict(names=["world"], parent=[-1], pos=[np.zeros(3)], quat=[np.array([1.0, 0, 0, 0])], jname=[None], jtype=[0],
                 jaxis=[np.array([0.0, 0, 1])], janchor=[np.zeros(3)])
    tris, tri_link, tri_robot, geom_names, geom_tris, cameras = [], [], [], [], [], {}

    def add_geom(el, link):
        refuse_orientation(el)
        gtype = el.get("type", "sphere")
        if gtype == "mesh":
            mname = el.get("mesh")
            if mname not in meshes:
                raise ValueError(f"{path}: geom refers to mesh {mname!r}, which <asset> does not define")
            file, scale = meshes[mname]
            if file not in stl_cache:
                stl_cache[file] = read_stl(file)
            local = stl_cache[file].astype(np.float64) * scale
        elif gtype in ("box", "sphere", "cylinder", "capsule"):
            local = primitive(gtype, _floats(el, "size", ()))
        else:
            raise ValueError(f"{path}: geom type {gtype!r} is not read (mesh, box, sphere, cylinder, capsule are)")
        R, p = quat_to_mat(_quat(el)), _floats(el, "pos", (0, 0, 0), 3)
        gname = el.get("name")
        tris.append((local @ R.T + p).astype(np.float32))
        tri_link.append(np.full(len(local), link, dtype=np.int32))
        tri_robot.append(np.full(len(local), bool(is_robot_geom(gname)), dtype=np.bool_))
        geom_names.append(gname)
        geom_tris.append(len(local))

    def add_children(parent_el, link):
        njoint = 0
        for el in parent_el:
            if el.tag == "geom":
                add_geom(el, link)
            elif el.tag == "camera":
                refuse_orientation(el)
                if el.get("mode", "fixed") != "fixed" or el.get("target") is not None:
                    raise ValueError(f"{path}: <camera mode={el.get('mode')!r}> is not read (fixed cameras are)")
                cname = el.get("name") or f"camera{len(cameras)}"
                cameras[cname] = MjcfCamera(cname, link, _floats(el, "pos", (0, 0, 0), 3), _quat(el),
                                            float(el.get("fovy", 45.0)))
            elif el.tag == "joint":
                if link == 0:
                    raise ValueError(f"{path}: a joint in <worldbody>")
                refuse_orientation(el)
                jtype = el.get("type", "hinge")
                if jtype not in ("hinge", "slide"):
                    raise ValueError(f"{path}: joint type {jtype!r} is not read (hinge and slide are)")
                if el.get("ref") is not None:
                    raise ValueError(f"{path}: <joint ref=...> is not read")
                njoint += 1
                if njoint > 1:
                    raise ValueError(f"{path}: body {links['names'][link]!r} has more than one joint")
                axis = _floats(el, "axis", (0, 0, 1), 3)
                if np.linalg.norm(axis) == 0:
                    raise ValueError(f"{path}: <joint axis> is zero")
                links["jname"][link] = el.get("name")
                links["jtype"][link] = JOINT_HINGE if jtype == "hinge" else JOINT_SLIDE
                links["jaxis"][link] = axis / np.linalg.norm(axis)
                links["janchor"][link] = _floats(el, "pos", (0, 0, 0), 3)
            elif el.tag == "body":
                refuse_orientation(el)
                child = len(links["names"])
                links["names"].append(el.get("name") or f"body{child}")
                links["parent"].append(link)
                links["pos"].append(_floats(el, "pos", (0, 0, 0), 3))
                links["quat"].append(_quat(el))
                links["jname"].append(None)
                links["jtype"].append(JOINT_NONE)
                links["jaxis"].append(np.array([0.0, 0, 1]))
                links["janchor"].append(np.zeros(3))
                add_children(el, child)
            elif el.tag not in _BODY_IGNORED:
                raise ValueError(f"{path}: <{el.tag}> inside <{parent_el.tag}> is not read")

    for wb in root.findall("worldbody"):
        add_children(wb, 0)
    L = len(links["names"])
    if L > MAX_LINKS:
        raise ValueError(f"{path}: {L} links, at most {MAX_LINKS} are rendered")
    have = [j for j in links["jname"] if j is not None]
    for j in joints:
        if have.count(j) != 1:
            raise ValueError(f"{path}: joint {j!r} is defined {have.count(j)} times")
    col = np.array([joints.index(j) if j in joints else -1 for j in links["jname"]], dtype=np.int32)
    return MjcfModel(
        name=name, link_names=links["names"], link_parent=np.array(links["parent"], dtype=np.int32),
        link_pos=np.stack(links["pos"]), link_quat=np.stack(links["quat"]), joint_names=links["jname"],
        joint_type=np.array(links["jtype"], dtype=np.int32), joint_axis=np.stack(links["jaxis"]),
        joint_anchor=np.stack(links["janchor"]), joint_col=col, joints=joints,
        tri=np.concatenate(tris) if tris else np.zeros((0, 3, 3), np.float32),
        tri_link=np.concatenate(tri_link) if tris else np.zeros(0, np.int32),
        tri_robot=np.concatenate(tri_robot) if tris else np.zeros(0, np.bool_),
        geom_names=geom_names, geom_tris=geom_tris, cameras=cameras, native_hw=tuple(int(x) for x in native_hw))


def opencv_camera_pose(ext, offset=(0, 0, 0)):
    """The reference's `MaskEnv.set_opencv_camera_pose` (base_mask_env.py:8-22): (pos, quat w x y z) of the MuJoCo camera
    that sees what the OpenCV camera with camera-to-world `ext` (4, 4) sees -- pos = ext[:3, 3] + offset, rotation =
    R(ext) Ry(180 deg)."""
    ext = np.asarray(ext, dtype=np.float64)
    if ext.shape != (4, 4):
        raise ValueError(f"camera extrinsics must be (4, 4), got {ext.shape}")
    flip = np.diag([-1.0, 1.0, -1.0])
    return ext[:3, 3] + np.asarray(offset, dtype=np.float64), mat_to_quat(ext[:3, :3] @ flip)
