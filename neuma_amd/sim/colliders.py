"""Colliders of the per-operator MPM path: rigid half-spaces, spheres and oriented boxes in simulation coordinates (the unit
cube, the same space as `sim_bounds`) that the grid update respects behind the box boundary condition.  No reference
counterpart (the reference's only obstacle is the box of mpm.py:373-429).  Definition of the response: include/neuma_hip.h;
fp64 restatement: neuma_amd/extras/colliders.py; kernels: csrc/nm_collide.h + k_grid_collide / k_grid_collide_bwd.

    sim:
      colliders:
        - {type: plane, point: [0.5, 0.3, 0.5], normal: [0.2, 1, 0], surface: friction, friction: 0.4}
        - {type: sphere, center: [0.5, 0.4, 0.5], radius: 0.08, surface: slip, velocity: [0, 0.1, 0]}
        - {type: box, center: [0.5, 0.2, 0.5], half: [0.2, 0.05, 0.2], euler_xyz_deg: [0, 0, 20], surface: sticky}

parse_colliders turns such a list into Plane / Sphere / Box objects (normals normalised and rotations built in fp64), with
the validation - and the messages - of nm_mpm_set_colliders; pack() makes the ctypes array that call takes.
"""
import ctypes as C
import math
from dataclasses import dataclass, field, replace
from typing import List, Sequence, Tuple

from .. import _lib as L

MAX_COLLIDERS = 8
SHAPES = {"plane": 0, "sphere": 1, "box": 2}
SURFACES = {"sticky": 0, "slip": 1, "friction": 2}
_IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)


def _vec3(value, what: str) -> Tuple[float, float, float]:
    try:
        v = tuple(float(a) for a in value)
    except TypeError:
        v = ()
    if len(v) != 3 or not all(math.isfinite(a) for a in v):
        raise ValueError(f"{what}: three finite numbers expected, got {value!r}")
    return v


@dataclass(frozen=True)
class _Collider:
    surface: str = "sticky"
    friction: float = 0.0
    velocity: Tuple[float, float, float] = (0.0, 0.0, 0.0)

    def _check_common(self) -> None:
        if self.surface not in SURFACES:
            raise ValueError(f"surface: unknown surface {self.surface!r} (one of {sorted(SURFACES)})")
        if not float(self.friction) >= 0.0:
            raise ValueError(f"friction: must not be negative (got {self.friction})")
        object.__setattr__(self, "friction", float(self.friction))
        object.__setattr__(self, "velocity", _vec3(self.velocity, "velocity"))

    @property
    def moving(self) -> bool:
        return any(a != 0.0 for a in self.velocity)


@dataclass(frozen=True)
class Plane(_Collider):
    """Half-space: solid where (p - point).normal < 0.  The normal is normalised (fp64) here."""
    shape_code = 0      # NM_COLLIDER_PLANE
    point: Tuple[float, float, float] = (0.0, 0.0, 0.0)
    normal: Tuple[float, float, float] = (0.0, 1.0, 0.0)

    def __post_init__(self) -> None:
        self._check_common()
        object.__setattr__(self, "point", _vec3(self.point, "point"))
        n = _vec3(self.normal, "normal")
        length = math.sqrt(sum(a * a for a in n))
        if not length > 0.0:
            raise ValueError("normal: not a unit vector (zero length)")
        object.__setattr__(self, "normal", tuple(a / length for a in n))

    def advanced(self, dt: float) -> "Plane":
        return replace(self, point=tuple(p + dt * v for p, v in zip(self.point, self.velocity)))


@dataclass(frozen=True)
class Sphere(_Collider):
    shape_code = 1      # NM_COLLIDER_SPHERE
    center: Tuple[float, float, float] = (0.0, 0.0, 0.0)
    radius: float = 0.0

    def __post_init__(self) -> None:
        self._check_common()
        object.__setattr__(self, "center", _vec3(self.center, "center"))
        if not float(self.radius) > 0.0:
            raise ValueError(f"radius: must be positive (got {self.radius})")
        object.__setattr__(self, "radius", float(self.radius))

    def advanced(self, dt: float) -> "Sphere":
        return replace(self, center=tuple(p + dt * v for p, v in zip(self.center, self.velocity)))


@dataclass(frozen=True)
class Box(_Collider):
    """Oriented box.  rot: row-major 3x3 rotation whose columns are the box's axes in simulation coordinates."""
    shape_code = 2      # NM_COLLIDER_BOX
    center: Tuple[float, float, float] = (0.0, 0.0, 0.0)
    half: Tuple[float, float, float] = (0.0, 0.0, 0.0)
    rot: Tuple[float, ...] = field(default=_IDENTITY)

    def __post_init__(self) -> None:
        self._check_common()
        object.__setattr__(self, "center", _vec3(self.center, "center"))
        half = _vec3(self.half, "half")
        if not all(a > 0.0 for a in half):
            raise ValueError(f"half: extents must be positive (got {half})")
        object.__setattr__(self, "half", half)
        rot = self.rot
        if len(rot) == 3 and all(hasattr(r, "__len__") for r in rot):
            rot = [a for r in rot for a in r]
        rot = tuple(float(a) for a in rot)
        if len(rot) != 9 or not all(math.isfinite(a) for a in rot):
            raise ValueError("rot: not orthonormal (nine finite numbers expected)")
        for a in range(3):
            for b in range(3):
                d = sum(rot[3 * r + a] * rot[3 * r + b] for r in range(3))
                if not abs(d - (1.0 if a == b else 0.0)) <= 1e-4:
                    raise ValueError("rot: not orthonormal")
        det = (rot[0] * (rot[4] * rot[8] - rot[5] * rot[7]) - rot[1] * (rot[3] * rot[8] - rot[5] * rot[6])
               + rot[2] * (rot[3] * rot[7] - rot[4] * rot[6]))
        if not det > 0.0:
            raise ValueError("rot: not orthonormal (a reflection: determinant -1)")
        object.__setattr__(self, "rot", rot)

    def advanced(self, dt: float) -> "Box":
        return replace(self, center=tuple(p + dt * v for p, v in zip(self.center, self.velocity)))


def euler_xyz_deg_to_rot(angles) -> Tuple[float, ...]:
    """R = Rz(c) Ry(b) Rx(a) for angles (a, b, c) in degrees about the fixed x, y, z axes, row-major, in fp64."""
    a, b, c = (math.radians(v) for v in _vec3(angles, "euler_xyz_deg"))
    ca, sa, cb, sb, cc, sc = math.cos(a), math.sin(a), math.cos(b), math.sin(b), math.cos(c), math.sin(c)
    return (cc * cb, cc * sb * sa - sc * ca, cc * sb * ca + sc * sa,
            sc * cb, sc * sb * sa + cc * ca, sc * sb * ca - cc * sa,
            -sb, cb * sa, cb * ca)


def parse_collider(node, index: int = 0):
    """One entry of `sim.colliders` (a dict; config nodes are dicts) -> Plane / Sphere / Box.  Errors name the entry and the field."""
    if isinstance(node, _Collider):
        return node
    kind = node.get("type")
    common = dict(surface=str(node.get("surface", "sticky")), friction=node.get("friction", 0.0),
                  velocity=node.get("velocity", (0.0, 0.0, 0.0)))
    try:
        if kind == "plane":
            return Plane(point=node.get("point", (0.0, 0.0, 0.0)), normal=node.get("normal", (0.0, 1.0, 0.0)), **common)
        if kind == "sphere":
            return Sphere(center=node.get("center", (0.0, 0.0, 0.0)), radius=node.get("radius", 0.0), **common)
        if kind == "box":
            euler, rot = node.get("euler_xyz_deg"), node.get("rot")
            if euler is not None and rot is not None:
                raise ValueError("rot: give either euler_xyz_deg or rot, not both")
            rot = euler_xyz_deg_to_rot(euler) if euler is not None else (_IDENTITY if rot is None else rot)
            return Box(center=node.get("center", (0.0, 0.0, 0.0)), half=node.get("half", (0.0, 0.0, 0.0)), rot=rot, **common)
        raise ValueError(f"shape: unknown shape {kind!r} (one of {sorted(SHAPES)})")
    except ValueError as e:
        raise ValueError(f"collider {index}: {e}") from None


def parse_colliders(nodes) -> List:
    """A `sim.colliders` list (dicts / config nodes / collider objects) -> validated collider objects, in order."""
    nodes = [] if nodes is None else list(nodes)
    if len(nodes) > MAX_COLLIDERS:
        raise ValueError(f"colliders: n = {len(nodes)} outside 0..{MAX_COLLIDERS}")
    return [parse_collider(n, i) for i, n in enumerate(nodes)]


def pack(colliders: Sequence):
    """ctypes array of nm_collider for nm_mpm_set_colliders (None for an empty list)."""
    if len(colliders) > MAX_COLLIDERS:
        raise ValueError(f"colliders: n = {len(colliders)} outside 0..{MAX_COLLIDERS}")
    if not colliders:
        return None
    arr = (L.nm_collider * len(colliders))()
    for out, c in zip(arr, colliders):
        out.shape = c.shape_code
        out.surface = SURFACES[c.surface]
        out.friction = c.friction
        out.velocity = (C.c_float * 3)(*c.velocity)
        out.center = (C.c_float * 3)(*(c.point if isinstance(c, Plane) else c.center))
        out.normal = (C.c_float * 3)(*(c.normal if isinstance(c, Plane) else (0.0, 0.0, 0.0)))
        out.radius = c.radius if isinstance(c, Sphere) else 0.0
        out.half = (C.c_float * 3)(*(c.half if isinstance(c, Box) else (0.0, 0.0, 0.0)))
        out.rot = (C.c_float * 9)(*(c.rot if isinstance(c, Box) else _IDENTITY))
    return arr


def describe(colliders: Sequence, drawn: bool = False) -> str:
    """One line per collider, for the entry points' start-up print.  drawn: the run draws them (neuma_amd/collider_draw.py)."""
    if not colliders:
        return "colliders: none"
    lines = [f"colliders: {len(colliders)} ({'drawn' if drawn else 'not drawn'} in renders)"]
    for i, c in enumerate(colliders):
        if isinstance(c, Plane):
            geo = f"plane point={c.point} normal={tuple(round(a, 6) for a in c.normal)}"
        elif isinstance(c, Sphere):
            geo = f"sphere center={c.center} radius={c.radius}"
        else:
            geo = f"box center={c.center} half={c.half} rot={tuple(round(a, 6) for a in c.rot)}"
        surf = c.surface + (f" mu={c.friction}" if c.surface == "friction" else "")
        lines.append(f"  [{i}] {geo} surface={surf} velocity={c.velocity}")
    return "\n".join(lines)


def refuse_in_training(cfg, what: str) -> None:
    """The training drivers step through the fused roll-out, which has no colliders: a config that sets `sim.colliders` raises."""
    sim = cfg.get("sim")
    if sim is not None and sim.get("colliders"):
        raise NotImplementedError(f"`sim.colliders` is set, but {what} trains through the fused roll-out and colliders act on the "
                                  "per-operator path only (python -m neuma_amd.inference / neuma_amd.render): remove sim.colliders")
