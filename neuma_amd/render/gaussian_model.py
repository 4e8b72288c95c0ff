"""3DGS parameter container: the accessors NeuMA's hot path reads, and the training surface of the static fit.
Mirrors /root/reference/modules/d3gs/scene/gaussian_model.py: activations 26-41, get_* 97-118
(get_xyz, get_features, get_opacity, get_covariance), with the covariance cached per scaling_modifier
(the reference recomputes it on every render call although it is constant); create_from_pcd 136-159,
training_setup / update_learning_rate 161-187, save_ply 203-220, reset_opacity 222-225 and the densification with its
optimiser-state surgery 326-480.  The bookkeeping is device-agnostic torch (it follows the parameters' device); only
create_from_pcd needs the GPU (distCUDA2 is the native k-NN search).  Every method that replaces a parameter drops the
covariance cache."""
import numpy as np
import torch
import torch.nn as nn
from torch import Tensor

from . import build_cov3D
from .general_utils import RGB2SH, build_rotation, get_expon_lr_func, inverse_sigmoid

_GROUPS = (("xyz", "_xyz"), ("f_dc", "_features_dc"), ("f_rest", "_features_rest"), ("opacity", "_opacity"),
           ("scaling", "_scaling"), ("rotation", "_rotation"))


class GaussianModel(object):
    def __init__(self, sh_degree: int):
        self.active_sh_degree = sh_degree
        self.max_sh_degree = sh_degree
        self._xyz = torch.empty(0)
        self._features_dc = torch.empty(0)
        self._features_rest = torch.empty(0)
        self._scaling = torch.empty(0)
        self._rotation = torch.empty(0)
        self._opacity = torch.empty(0)
        self._cov_cache = {}
        self.max_radii2D = torch.empty(0)
        self.xyz_gradient_accum = torch.empty(0)
        self.denom = torch.empty(0)
        self.optimizer = None
        self.percent_dense = 0
        self.spatial_lr_scale = 0

    def set_params(self, xyz: Tensor, features_dc: Tensor, features_rest: Tensor, scaling: Tensor, rotation: Tensor,
                   opacity: Tensor) -> "GaussianModel":
        """xyz (K,3); features_dc (K,1,3); features_rest (K,(deg+1)^2-1,3); scaling = log-scales (K,3);
        rotation = quaternions (K,4) (r,x,y,z); opacity = logits (K,1) — the PLY-side parametrisation."""
        self._xyz, self._features_dc, self._features_rest = xyz, features_dc, features_rest
        self._scaling, self._rotation, self._opacity = scaling, rotation, opacity
        self._cov_cache = {}
        return self

    @property
    def get_scaling(self):
        return torch.exp(self._scaling)

    @property
    def get_rotation(self):
        return torch.nn.functional.normalize(self._rotation)

    @property
    def get_xyz(self):
        return self._xyz

    @property
    def get_features(self):
        return torch.cat((self._features_dc, self._features_rest), dim=1)

    @property
    def get_opacity(self):
        return torch.sigmoid(self._opacity)

    def get_covariance(self, scaling_modifier=1):
        key = float(scaling_modifier)
        if key not in self._cov_cache:
            with torch.no_grad():
                self._cov_cache[key] = build_cov3D(self.get_scaling, self._rotation, key).contiguous()
        return self._cov_cache[key]

    # ------------------------------------------------------------------ training surface

    def invalidate(self) -> None:
        """Drop the covariance cache: to be called after the parameters changed in place (an optimiser step)."""
        self._cov_cache = {}

    def capture(self):
        return (self.active_sh_degree, self._xyz, self._features_dc, self._features_rest, self._scaling, self._rotation,
                self._opacity, self.max_radii2D, self.xyz_gradient_accum, self.denom, self.optimizer.state_dict(),
                self.spatial_lr_scale)

    def restore(self, model_args, training_args) -> None:
        (self.active_sh_degree, self._xyz, self._features_dc, self._features_rest, self._scaling, self._rotation, self._opacity,
         self.max_radii2D, accum, denom, opt_dict, self.spatial_lr_scale) = model_args
        self.invalidate()
        self.training_setup(training_args)
        self.xyz_gradient_accum, self.denom = accum, denom
        self.optimizer.load_state_dict(opt_dict)

    def get_scale_regularization(self, max_gauss_ratio: float):
        s = self.get_scaling
        ratio = s.amax(dim=-1) / s.amin(dim=-1)
        return torch.mean(torch.clamp_min(ratio, max_gauss_ratio) - max_gauss_ratio)

    def oneupSHdegree(self) -> None:
        if self.active_sh_degree < self.max_sh_degree:
            self.active_sh_degree += 1

    def create_from_pcd(self, points, colors, spatial_lr_scale: float, device="cuda") -> "GaussianModel":
        """points (N,3), colors (N,3) in [0,1] (arrays or tensors): isotropic scales sqrt(distCUDA2), opacity 0.1, identity
        rotations, DC colour RGB2SH(colors), higher SH rows zero.  Training starts at SH degree 0."""
        from .simple_knn import distCUDA2
        self.spatial_lr_scale = spatial_lr_scale
        xyz = torch.as_tensor(np.asarray(points.detach().cpu() if isinstance(points, Tensor) else points)).float().to(device)
        rgb = torch.as_tensor(np.asarray(colors.detach().cpu() if isinstance(colors, Tensor) else colors)).float().to(device)
        n = xyz.shape[0]
        feats = torch.zeros(n, (self.max_sh_degree + 1) ** 2, 3, dtype=torch.float32, device=xyz.device)
        feats[:, 0, :] = RGB2SH(rgb)
        dist2 = torch.clamp_min(distCUDA2(xyz), 0.0000001)
        scales = torch.log(torch.sqrt(dist2))[..., None].repeat(1, 3)
        rots = torch.zeros(n, 4, device=xyz.device)
        rots[:, 0] = 1
        logits = inverse_sigmoid(0.1 * torch.ones(n, 1, dtype=torch.float32, device=xyz.device))
        self.active_sh_degree = 0
        self._xyz = nn.Parameter(xyz.contiguous().requires_grad_(True))
        self._features_dc = nn.Parameter(feats[:, 0:1].contiguous().requires_grad_(True))
        self._features_rest = nn.Parameter(feats[:, 1:].contiguous().requires_grad_(True))
        self._scaling = nn.Parameter(scales.contiguous().requires_grad_(True))
        self._rotation = nn.Parameter(rots.requires_grad_(True))
        self._opacity = nn.Parameter(logits.requires_grad_(True))
        self.max_radii2D = torch.zeros(n, device=xyz.device)
        self.invalidate()
        return self

    def training_setup(self, args) -> None:
        """Adam (eps 1e-15) over the six parameter groups; `args` carries percent_dense, position_lr_init / _final /
        _delay_mult / _max_steps, feature_lr, opacity_lr, scaling_lr, rotation_lr."""
        dev = self._xyz.device
        for _, attr in _GROUPS:                       # tensors handed over by set_params become leaves the optimiser owns
            t = getattr(self, attr)
            if not isinstance(t, nn.Parameter):
                setattr(self, attr, nn.Parameter(t.detach().clone().contiguous().requires_grad_(True)))
        self.invalidate()
        n = self._xyz.shape[0]
        self.percent_dense = args.percent_dense
        self.xyz_gradient_accum = torch.zeros(n, 1, device=dev)
        self.denom = torch.zeros(n, 1, device=dev)
        if self.max_radii2D.shape[0] != n:
            self.max_radii2D = torch.zeros(n, device=dev)
        lrs = {"xyz": args.position_lr_init * self.spatial_lr_scale, "f_dc": args.feature_lr, "f_rest": args.feature_lr / 20.0,
               "opacity": args.opacity_lr, "scaling": args.scaling_lr, "rotation": args.rotation_lr}
        groups = [{"params": [getattr(self, attr)], "lr": lrs[name], "name": name} for name, attr in _GROUPS]
        self.optimizer = torch.optim.Adam(groups, lr=0.0, eps=1e-15)
        self.xyz_scheduler_args = get_expon_lr_func(lr_init=args.position_lr_init * self.spatial_lr_scale,
                                                    lr_final=args.position_lr_final * self.spatial_lr_scale,
                                                    lr_delay_mult=args.position_lr_delay_mult,
                                                    max_steps=args.position_lr_max_steps)

    def update_learning_rate(self, iteration):
        for group in self.optimizer.param_groups:
            if group["name"] == "xyz":
                group["lr"] = lr = self.xyz_scheduler_args(iteration)
                return lr

    def save_ply(self, path) -> None:
        from ..io import save_gaussians_ply
        save_gaussians_ply(self, path)

    # ---- optimiser-state surgery: every group holds one parameter; `rows` maps the old parameter and each of its Adam moments
    #      to the new one

    def _rebuild(self, rows) -> None:
        for group in self.optimizer.param_groups:
            old = group["params"][0]
            state = self.optimizer.state.pop(old, None)
            new = nn.Parameter(rows(group["name"], old.detach(), False).contiguous().requires_grad_(True))
            if state is not None:
                state["exp_avg"] = rows(group["name"], state["exp_avg"], True).contiguous()
                state["exp_avg_sq"] = rows(group["name"], state["exp_avg_sq"], True).contiguous()
                self.optimizer.state[new] = state
            group["params"][0] = new
            setattr(self, dict(_GROUPS)[group["name"]], new)
        self.invalidate()

    def replace_tensor_to_optimizer(self, tensor: Tensor, name: str) -> None:
        """Group `name` gets `tensor` as its parameter, with zeroed Adam moments."""
        def rows(group, t, is_state):
            if group != name:
                return t
            return torch.zeros_like(tensor) if is_state else tensor.detach()
        self._rebuild(rows)

    def reset_opacity(self) -> None:
        op = self.get_opacity.detach()
        self.replace_tensor_to_optimizer(inverse_sigmoid(torch.min(op, torch.ones_like(op) * 0.01)), "opacity")

    def prune_points(self, mask: Tensor) -> None:
        """Remove the rows where `mask` is True from the parameters, their Adam moments and the densification statistics."""
        keep = ~mask
        self._rebuild(lambda group, t, is_state: t[keep])
        self.xyz_gradient_accum = self.xyz_gradient_accum[keep]
        self.denom = self.denom[keep]
        self.max_radii2D = self.max_radii2D[keep]

    def densification_postfix(self, new_xyz, new_features_dc, new_features_rest, new_opacities, new_scaling, new_rotation) -> None:
        """Append rows (zero Adam moments) and restart the densification statistics."""
        ext = {"xyz": new_xyz, "f_dc": new_features_dc, "f_rest": new_features_rest, "opacity": new_opacities,
               "scaling": new_scaling, "rotation": new_rotation}

        def rows(group, t, is_state):
            e = ext[group].detach()
            return torch.cat((t, torch.zeros_like(e) if is_state else e), dim=0)
        self._rebuild(rows)
        n, dev = self._xyz.shape[0], self._xyz.device
        self.xyz_gradient_accum = torch.zeros(n, 1, device=dev)
        self.denom = torch.zeros(n, 1, device=dev)
        self.max_radii2D = torch.zeros(n, device=dev)

    def densify_and_split(self, grads: Tensor, grad_threshold: float, scene_extent: float, N: int = 2) -> None:
        """Large Gaussians (max scale > percent_dense * extent) with grad >= threshold are replaced by N samples of themselves,
        scales divided by 0.8 N."""
        n = self._xyz.shape[0]
        dev = self._xyz.device
        padded = torch.zeros(n, device=dev)
        padded[:grads.shape[0]] = grads.reshape(-1)
        sel = (padded >= grad_threshold) & (self.get_scaling.max(dim=1).values > self.percent_dense * scene_extent)
        with torch.no_grad():
            stds = self.get_scaling[sel].repeat(N, 1)
            samples = torch.normal(mean=torch.zeros_like(stds), std=stds)
            R = build_rotation(self._rotation[sel]).repeat(N, 1, 1)
            new_xyz = torch.bmm(R, samples.unsqueeze(-1)).squeeze(-1) + self._xyz[sel].repeat(N, 1)
            new_scaling = torch.log(self.get_scaling[sel].repeat(N, 1) / (0.8 * N))
            new = (new_xyz, self._features_dc[sel].repeat(N, 1, 1), self._features_rest[sel].repeat(N, 1, 1),
                   self._opacity[sel].repeat(N, 1), new_scaling, self._rotation[sel].repeat(N, 1))
        self.densification_postfix(*new)
        self.prune_points(torch.cat((sel, torch.zeros(N * int(sel.sum()), device=dev, dtype=torch.bool))))

    def densify_and_clone(self, grads: Tensor, grad_threshold: float, scene_extent: float) -> None:
        """Small Gaussians (max scale <= percent_dense * extent) with |grad| >= threshold are duplicated."""
        sel = (torch.norm(grads, dim=-1) >= grad_threshold) & \
              (self.get_scaling.max(dim=1).values <= self.percent_dense * scene_extent)
        self.densification_postfix(self._xyz[sel], self._features_dc[sel], self._features_rest[sel], self._opacity[sel],
                                   self._scaling[sel], self._rotation[sel])

    def densify_and_prune(self, max_grad: float, min_opacity: float, extent: float, max_screen_size) -> None:
        grads = self.xyz_gradient_accum / self.denom
        grads[grads.isnan()] = 0.0
        self.densify_and_clone(grads, max_grad, extent)
        self.densify_and_split(grads, max_grad, extent)
        prune = (self.get_opacity < min_opacity).squeeze(-1)
        if max_screen_size:
            prune = prune | (self.max_radii2D > max_screen_size) | (self.get_scaling.max(dim=1).values > 0.1 * extent)
        self.prune_points(prune)

    def add_densification_stats(self, viewspace_grad: Tensor, update_filter: Tensor) -> None:
        """viewspace_grad: dL/dmeans2D (K, >= 2) of the last render; update_filter: its `radii > 0`.  Masked arithmetic rather
        than masked indexing: nothing is read back to the host."""
        vis = update_filter.unsqueeze(-1)
        norm = torch.norm(viewspace_grad[:, :2], dim=-1, keepdim=True)
        self.xyz_gradient_accum += torch.where(vis, norm, torch.zeros_like(norm))
        self.denom += vis.to(self.denom.dtype)
