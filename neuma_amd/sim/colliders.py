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

Mesh colliders: a closed triangle mesh as an obstacle, through its signed distance field on a lattice (neuma_amd/mesh_sdf.py;
response: include/neuma_hip.h "Field colliders", csrc/nm_collide_field.h, extras/colliders.py apply_field_collider).

        - {type: mesh, path: bowl.obj, scale: 0.3, euler_xyz_deg: [0, 0, 15], translate: [0.5, 0.2, 0.5],
           resolution: 64, surface: friction, friction: 0.4, velocity: [0, 0, 0]}

The mesh (`path`: .obj / .ply, or `verts` / `tris` arrays from code) is mapped by p_s = scale R p_mesh + translate in fp64 on
the host; `resolution` cells along the longest axis of its box (or a `spacing`), `margin_cells` (2) cells of margin.  Mesh entries
come after all analytic entries (list order is the order of application, and field colliders act behind the analytic ones), at
most MAX_FIELD_COLLIDERS of them.  parse_colliders returns them as MeshCollider objects behind the analytic ones; a model builds
each one's field once (MeshCollider.build -> FieldCollider, which is what nm_mpm_set_field_colliders takes: pack_fields).  A
FieldCollider can also be made from any signed distance field directly.  pack() stays what it was: analytic colliders only.

Rigid bodies (include/neuma_hip.h "Rigid bodies"; fp64 restatement: neuma_amd/extras/rigid.py): a sphere or box entry may be a body
that the material and gravity move, on the device, forward only.

        - {type: sphere, center: [0.5, 0.7, 0.5], radius: 0.08, surface: sticky, dynamic: true, density: 4000}
        - {type: box, center: [0.5, 0.5, 0.5], half: [0.2, 0.02, 0.05], kinematic: true, angular_velocity: [0, 6, 0]}

`dynamic: true` needs `mass` or `density` (simulation units: the unit cube, rho * vol masses - mass = density * volume);
`kinematic: true` keeps `velocity` and `angular_velocity` whatever pushes it (a paddle; mass defaults to 1 and moves nothing);
`angular_velocity` is in simulation axes; `gravity: false` switches the model's gravity off for the body.  The entry parses into
its Sphere / Box with a RigidBody record in `.body`; pack_bodies() makes the array nm_mpm_set_rigid_bodies takes.
"""
import ctypes as C
import math
from dataclasses import dataclass, field, replace
from typing import List, Optional, Sequence, Tuple

from .. import _lib as L

MAX_COLLIDERS = 8
MAX_FIELD_COLLIDERS = 4
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

    body = None      # Sphere / Box: the RigidBody record of an entry that is a rigid body

    @property
    def moving(self) -> bool:
        """a prescribed mover, which the host advances (a rigid body is moved on the device instead)"""
        return self.body is None and any(a != 0.0 for a in self.velocity)


@dataclass(frozen=True)
class RigidBody:
    """What makes a sphere or box entry a rigid body: mass M, body-frame principal inertia I_b, the initial angular velocity
    (simulation axes), whether the model's gravity acts on it, and whether it is kinematic (keeps v and w, ignores impulses)."""
    mass: float = 1.0
    inertia: Tuple[float, float, float] = (1.0, 1.0, 1.0)
    angular_velocity: Tuple[float, float, float] = (0.0, 0.0, 0.0)
    gravity: bool = True
    kinematic: bool = False

    def __post_init__(self) -> None:
        if not (float(self.mass) > 0.0 and math.isfinite(float(self.mass))):
            raise ValueError(f"mass: must be positive (got {self.mass})")
        object.__setattr__(self, "mass", float(self.mass))
        inertia = _vec3(self.inertia, "inertia")
        if not all(a > 0.0 for a in inertia):
            raise ValueError(f"inertia: must be positive (got {inertia})")
        object.__setattr__(self, "inertia", inertia)
        object.__setattr__(self, "angular_velocity", _vec3(self.angular_velocity, "angular_velocity"))

    @property
    def flags(self) -> int:
        return (1 if self.kinematic else 0) | (0 if self.gravity else 2)      # NM_RIGID_KINEMATIC | NM_RIGID_NO_GRAVITY


def volume(c) -> float:
    """of a Sphere or Box"""
    if isinstance(c, Sphere):
        return 4.0 / 3.0 * math.pi * c.radius ** 3
    return 8.0 * c.half[0] * c.half[1] * c.half[2]


def principal_inertia(c, mass: float) -> Tuple[float, float, float]:
    """Body-frame principal inertia of a solid Sphere (2/5 M r^2) or Box (M/3 (hy^2 + hz^2, hx^2 + hz^2, hx^2 + hy^2))."""
    if isinstance(c, Sphere):
        i = 0.4 * mass * c.radius ** 2
        return (i, i, i)
    hx, hy, hz = (a * a for a in c.half)
    return (mass / 3.0 * (hy + hz), mass / 3.0 * (hx + hz), mass / 3.0 * (hx + hy))


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
    body: Optional[RigidBody] = None

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
    body: Optional[RigidBody] = None

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


@dataclass(frozen=True, eq=False)
class FieldCollider(_Collider):
    """An obstacle given as a signed distance field phi (nx, ny, nz; negative inside) on the lattice origin + index * spacing, in
    simulation coordinates.  phi: an fp32 tensor on the model's device for a simulation (the model keeps it alive); any array for
    the fp64 definition (extras/colliders.py).  origin is the position of node (0,0,0) NOW; `source`: the MeshCollider it was
    built from, if any."""
    phi: object = None
    origin: Tuple[float, float, float] = (0.0, 0.0, 0.0)
    spacing: float = 0.0
    dims: Tuple[int, int, int] = (0, 0, 0)
    source: Optional["MeshCollider"] = None

    def __post_init__(self) -> None:
        self._check_common()
        object.__setattr__(self, "origin", _vec3(self.origin, "origin"))
        if not (float(self.spacing) > 0.0 and math.isfinite(float(self.spacing))):
            raise ValueError(f"spacing: must be positive (got {self.spacing})")
        object.__setattr__(self, "spacing", float(self.spacing))
        dims = tuple(int(d) for d in self.dims)
        if len(dims) != 3 or min(dims) < 2:
            raise ValueError(f"dims: every lattice size must be >= 2 (got {self.dims})")
        if dims[0] * dims[1] * dims[2] > (1 << 27):
            raise ValueError(f"dims: more than 2^27 nodes ({dims})")
        object.__setattr__(self, "dims", dims)
        if self.phi is None or tuple(self.phi.shape) != dims:
            raise ValueError(f"phi: an array of shape {dims} expected")

    def advanced(self, dt: float) -> "FieldCollider":
        return replace(self, origin=tuple(p + dt * v for p, v in zip(self.origin, self.velocity)))


@dataclass(frozen=True, eq=False)
class MeshCollider(_Collider):
    """A closed triangle mesh as an obstacle: verts (n, 3) fp64 ALREADY in simulation coordinates, tris (m, 3).  build() makes the
    FieldCollider a model steps against."""
    verts: object = None
    tris: object = None
    path: Optional[str] = None
    resolution: int = 64
    spacing: Optional[float] = None
    margin_cells: int = 2

    def __post_init__(self) -> None:
        import numpy as np
        from ..extras import mesh_sdf
        self._check_common()
        v = np.asarray(self.verts, dtype=np.float64)
        if v.ndim != 2 or v.shape[1] != 3 or len(v) == 0 or not np.isfinite(v).all():
            raise ValueError("verts: an (n, 3) array of finite numbers expected")
        t = np.asarray(self.tris)
        if t.ndim != 2 or t.shape[1] != 3 or not np.issubdtype(t.dtype, np.integer):
            raise ValueError("tris: an (m, 3) array of vertex indices expected")
        object.__setattr__(self, "verts", v)
        object.__setattr__(self, "tris", mesh_sdf.check_closed_mesh(v, t))          # ValueError: open (edge count) / inverted
        if self.spacing is None and not int(self.resolution) >= 1:
            raise ValueError(f"resolution: must be >= 1 (got {self.resolution})")
        if self.spacing is not None and not (float(self.spacing) > 0.0 and math.isfinite(float(self.spacing))):
            raise ValueError(f"spacing: must be positive (got {self.spacing})")
        if not int(self.margin_cells) >= 0:
            raise ValueError(f"margin_cells: must not be negative (got {self.margin_cells})")
        mesh_sdf.field_lattice(v, self.spacing, self.resolution, self.margin_cells)   # ValueError: a lattice beyond 2^27 nodes

    def build(self, device) -> FieldCollider:
        """The signed distance field on `device` (a GPU: nm_mesh_distance + nm_points_in_mesh; "cpu": numpy fp64)."""
        from .. import mesh_sdf
        f = mesh_sdf.build_mesh_field(self.verts, self.tris, self.spacing, self.resolution, self.margin_cells, device)
        return FieldCollider(surface=self.surface, friction=self.friction, velocity=self.velocity, phi=f.phi, origin=f.origin,
                             spacing=f.spacing, dims=f.dims, source=self)


def _mesh_collider(node, common) -> MeshCollider:
    import numpy as np
    path, verts, tris = node.get("path"), node.get("verts"), node.get("tris")
    if (path is None) == (verts is None or tris is None):
        raise ValueError("path: give either a mesh file (path) or verts and tris arrays")
    if path is not None:
        from ..extras import mesh_sampling
        low = str(path).lower()
        if low.endswith(".obj"):
            verts, tris = mesh_sampling.read_obj_mesh(path)
        elif low.endswith(".ply"):
            verts, tris = mesh_sampling.read_ply_mesh(path)
        else:
            raise ValueError(f"path: an .obj or .ply mesh expected, got {path!r}")
    v = np.asarray(verts, dtype=np.float64)
    if v.ndim != 2 or v.shape[1] != 3:
        raise ValueError("verts: an (n, 3) array of finite numbers expected")
    scale = float(node.get("scale", 1.0))
    if not (scale > 0.0 and math.isfinite(scale)):
        raise ValueError(f"scale: must be positive (got {node.get('scale')})")
    R = np.asarray(euler_xyz_deg_to_rot(node.get("euler_xyz_deg", (0.0, 0.0, 0.0))), dtype=np.float64).reshape(3, 3)
    tr = np.asarray(_vec3(node.get("translate", (0.0, 0.0, 0.0)), "translate"), dtype=np.float64)
    spacing = node.get("spacing")
    return MeshCollider(verts=scale * (v @ R.T) + tr, tris=tris, path=None if path is None else str(path),
                        resolution=int(node.get("resolution", 64)), spacing=None if spacing is None else float(spacing),
                        margin_cells=int(node.get("margin_cells", 2)), **common)


def is_field(c) -> bool:
    """a mesh / field collider (applied behind the analytic ones) rather than a Plane / Sphere / Box"""
    return isinstance(c, (MeshCollider, FieldCollider))


def euler_xyz_deg_to_rot(angles) -> Tuple[float, ...]:
    """R = Rz(c) Ry(b) Rx(a) for angles (a, b, c) in degrees about the fixed x, y, z axes, row-major, in fp64."""
    a, b, c = (math.radians(v) for v in _vec3(angles, "euler_xyz_deg"))
    ca, sa, cb, sb, cc, sc = math.cos(a), math.sin(a), math.cos(b), math.sin(b), math.cos(c), math.sin(c)
    return (cc * cb, cc * sb * sa - sc * ca, cc * sb * ca + sc * sa,
            sc * cb, sc * sb * sa + cc * ca, sc * sb * ca - cc * sa,
            -sb, cb * sa, cb * ca)


_BODY_KEYS = ("mass", "density", "angular_velocity", "gravity")


def _rigid_body(node, shape) -> Optional[RigidBody]:
    """The RigidBody record of one `sim.colliders` entry (None: a static or prescribed collider); shape: its Sphere / Box."""
    dynamic, kinematic = bool(node.get("dynamic", False)), bool(node.get("kinematic", False))
    if not (dynamic or kinematic):
        for key in _BODY_KEYS:
            if node.get(key) is not None:
                raise ValueError(f"{key}: only a rigid body takes it (set dynamic: true or kinematic: true)")
        return None
    if dynamic and kinematic:
        raise ValueError("kinematic: give either dynamic or kinematic, not both")
    which = "dynamic" if dynamic else "kinematic"
    if not isinstance(shape, (Sphere, Box)):
        raise ValueError(f"{which}: only a sphere or a box can be a rigid body (got {node.get('type')})")
    mass, density = node.get("mass"), node.get("density")
    if mass is not None and density is not None:
        raise ValueError("density: give either mass or density, not both")
    if density is not None:
        if not (float(density) > 0.0 and math.isfinite(float(density))):
            raise ValueError(f"density: must be positive (got {density})")
        mass = float(density) * volume(shape)
    elif mass is None:
        if dynamic:
            raise ValueError("mass: a dynamic body needs mass or density")
        mass = 1.0
    if not (float(mass) > 0.0 and math.isfinite(float(mass))):
        raise ValueError(f"mass: must be positive (got {mass})")
    return RigidBody(mass=float(mass), inertia=principal_inertia(shape, float(mass)),
                     angular_velocity=node.get("angular_velocity", (0.0, 0.0, 0.0)), gravity=bool(node.get("gravity", True)),
                     kinematic=kinematic)


def parse_collider(node, index: int = 0):
    """One entry of `sim.colliders` (a dict; config nodes are dicts) -> Plane / Sphere / Box / MeshCollider.  Errors name the entry
    and the field."""
    if isinstance(node, _Collider):
        return node
    kind = node.get("type")
    common = dict(surface=str(node.get("surface", "sticky")), friction=node.get("friction", 0.0),
                  velocity=node.get("velocity", (0.0, 0.0, 0.0)))
    try:
        if kind == "plane":
            shape = Plane(point=node.get("point", (0.0, 0.0, 0.0)), normal=node.get("normal", (0.0, 1.0, 0.0)), **common)
            _rigid_body(node, shape)
            return shape
        if kind == "sphere":
            shape = Sphere(center=node.get("center", (0.0, 0.0, 0.0)), radius=node.get("radius", 0.0), **common)
            body = _rigid_body(node, shape)
            return shape if body is None else replace(shape, body=body)
        if kind == "box":
            euler, rot = node.get("euler_xyz_deg"), node.get("rot")
            if euler is not None and rot is not None:
                raise ValueError("rot: give either euler_xyz_deg or rot, not both")
            rot = euler_xyz_deg_to_rot(euler) if euler is not None else (_IDENTITY if rot is None else rot)
            shape = Box(center=node.get("center", (0.0, 0.0, 0.0)), half=node.get("half", (0.0, 0.0, 0.0)), rot=rot, **common)
            body = _rigid_body(node, shape)
            return shape if body is None else replace(shape, body=body)
        if kind == "mesh":
            _rigid_body(node, None)
            return _mesh_collider(node, common)
        raise ValueError(f"shape: unknown shape {kind!r} (one of {sorted(SHAPES) + ['mesh']})")
    except ValueError as e:
        raise ValueError(f"collider {index}: {e}") from None


def parse_colliders(nodes) -> List:
    """A `sim.colliders` list (dicts / config nodes / collider objects) -> validated collider objects, in order: the analytic ones
    (at most MAX_COLLIDERS), then the mesh / field colliders (at most MAX_FIELD_COLLIDERS).  A mesh entry in front of an analytic
    one raises ValueError naming the entry: list order is the order of application."""
    nodes = [] if nodes is None else list(nodes)
    kinds = [is_field(n) or (not isinstance(n, _Collider) and n.get("type") == "mesh") for n in nodes]
    n_analytic, n_field = kinds.count(False), kinds.count(True)
    if n_analytic > MAX_COLLIDERS:
        raise ValueError(f"colliders: n = {n_analytic} outside 0..{MAX_COLLIDERS}")
    if n_field > MAX_FIELD_COLLIDERS:
        raise ValueError(f"colliders: {n_field} mesh colliders, at most {MAX_FIELD_COLLIDERS}")
    for i, k in enumerate(kinds):
        if k and not all(kinds[i:]):
            raise ValueError(f"collider {i}: a mesh collider in front of an analytic one (mesh entries come after all plane / sphere / "
                             "box entries: they are applied behind them)")
    return [parse_collider(n, i) for i, n in enumerate(nodes)]


def split(colliders: Sequence) -> Tuple[List, List]:
    """(analytic colliders, mesh / field colliders) of a parsed list, each in order"""
    return [c for c in colliders if not is_field(c)], [c for c in colliders if is_field(c)]


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


def bodies_of(colliders: Sequence) -> List[Tuple[int, RigidBody]]:
    """(index, RigidBody) of the entries of an analytic list that are rigid bodies, in list order"""
    return [(i, c.body) for i, c in enumerate(colliders) if c.body is not None]


def pack_bodies(colliders: Sequence):
    """ctypes array of nm_rigid_body for nm_mpm_set_rigid_bodies, one per body entry of the analytic list (None without bodies)."""
    bodies = bodies_of(colliders)
    if not bodies:
        return None
    arr = (L.nm_rigid_body * len(bodies))()
    for out, (i, b) in zip(arr, bodies):
        out.collider = i
        out.flags = b.flags
        out.mass = b.mass
        out.inertia = (C.c_double * 3)(*b.inertia)
        out.angular_velocity = (C.c_double * 3)(*b.angular_velocity)
    return arr


def pack_fields(fields: Sequence):
    """ctypes array of nm_field_collider for nm_mpm_set_field_colliders (None for an empty list).  Every phi must be a contiguous
    fp32 tensor on the GPU; the caller keeps the tensors alive while the handle holds the set."""
    if len(fields) > MAX_FIELD_COLLIDERS:
        raise ValueError(f"field colliders: n = {len(fields)} outside 0..{MAX_FIELD_COLLIDERS}")
    if not fields:
        return None
    arr = (L.nm_field_collider * len(fields))()
    for out, c in zip(arr, fields):
        out.surface = SURFACES[c.surface]
        out.friction = c.friction
        out.velocity = (C.c_float * 3)(*c.velocity)
        out.origin = (C.c_float * 3)(*c.origin)
        out.spacing = c.spacing
        out.dims = (C.c_int32 * 3)(*c.dims)
        out.phi = L.ptr(c.phi)
    return arr


def describe_fields(fields: Sequence, draw_wanted: bool = False, drawn: bool = False) -> str:
    """One line per mesh / field collider: path, triangle count, lattice, surface.  drawn: the run draws them (draw_mesh_colliders);
    draw_wanted: it draws the analytic ones only."""
    note = " (drawn in renders)" if drawn else (" (mesh colliders are not drawn in renders)" if draw_wanted else "")
    lines = [f"mesh colliders: {len(fields)}" + note]
    for i, c in enumerate(fields):
        src = c if isinstance(c, MeshCollider) else c.source
        what = f"mesh path={src.path} triangles={len(src.tris)}" if src is not None else "field"
        lat = f" lattice={c.dims[0]}x{c.dims[1]}x{c.dims[2]} spacing={c.spacing:.6g}" if isinstance(c, FieldCollider) else ""
        surf = c.surface + (f" mu={c.friction}" if c.surface == "friction" else "")
        lines.append(f"  [{i}] {what}{lat} surface={surf} velocity={c.velocity}")
    return "\n".join(lines)


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
        if c.body is not None:
            b = c.body
            lines.append(f"      rigid body: {'kinematic' if b.kinematic else 'dynamic'} mass={b.mass:.6g} "
                         f"inertia={tuple(round(a, 9) for a in b.inertia)} angular_velocity={b.angular_velocity} "
                         f"gravity={'on' if b.gravity else 'off'}")
    return "\n".join(lines)


def refuse_in_training(cfg, what: str) -> None:
    """The training drivers step through the fused roll-out, which has no colliders: a config that sets `sim.colliders` raises."""
    sim = cfg.get("sim")
    if sim is not None and sim.get("colliders"):
        raise NotImplementedError(f"`sim.colliders` is set, but {what} trains through the fused roll-out and colliders act on the "
                                  "per-operator path only (python -m neuma_amd.inference / neuma_amd.render): remove sim.colliders")
