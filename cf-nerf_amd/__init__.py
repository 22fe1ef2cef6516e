"""cfnerf_amd - MI355X-native (gfx950) CF-NeRF ray-batch hot path behind the reference's Python interface.

Import as ``import cfnerf_amd`` (repo-root shim; the directory name ``cf-nerf_amd`` is not an identifier).
"""
from . import _lib  # noqa: F401
from . import train  # noqa: F401
from . import evaluate  # noqa: F401
from .evaluate import (OccupancyGrid, OccupancySampler, ause_fused, calibration, density_grid, gather_rows, image_metrics, render_path_train,  # noqa: F401
                       render_uncertainty, row_shard, sparsification_curves, sparsification_plot)
from . import data  # noqa: F401
from .data import DepthRayPool, RayPool  # noqa: F401
from .api import default_args, save_checkpoint  # noqa: F401
from .api import (Embedder, NeRF_Flows, batchify, batchify_rays, create_nerf, get_embedder, get_rays, get_rays_by_coord, img2mse,  # noqa: F401
                  k_scores, mse2psnr, ndc_rays, pack_rays, param_layout, raw2outputs, ray_regularizers, render, render_geometry, render_rays, render_rays_warped, run_network, ssim, t_vals_table, warp_z_vals)

__all__ = ["Embedder", "NeRF_Flows", "batchify", "batchify_rays", "create_nerf", "get_embedder", "get_rays", "get_rays_by_coord",
           "img2mse", "mse2psnr", "ndc_rays", "param_layout", "raw2outputs", "render", "render_rays", "run_network",
           "t_vals_table", "render_path_train", "render_uncertainty", "gather_rows", "row_shard", "sparsification_plot", "sparsification_curves", "ause_fused", "image_metrics", "RayPool", "DepthRayPool", "save_checkpoint", "default_args", "render_geometry", "density_grid", "pack_rays",
           "OccupancyGrid", "OccupancySampler", "warp_z_vals", "render_rays_warped", "ray_regularizers", "k_scores", "calibration", "ssim"]
