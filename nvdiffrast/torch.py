"""`nvdiffrast.torch` as the reference uses it: `texture` in cube mode (street_gaussian/models/sky_cubemap.py:102, 120 and
205), through the HIP kernel of street_crafter_amd/csrc/cubemap.hip.

    dr.texture(cube[None].sigmoid(), rays_d[None], filter_mode='linear', boundary_mode='cube')            :102  [1,H,W,3]
    dr.texture(cube[None].sigmoid(), rays_d[None, None], filter_mode='linear', boundary_mode='cube')      :120  [1,1,N,3]
    dr.texture(cubemap[None], reflvec[None].contiguous(), filter_mode='linear', boundary_mode='cube')     :205  [1,r,2r,3]

run unchanged.  The sampling rule is the one street_crafter_amd/cubemap.py states; bit parity with nvdiffrast's own CUDA
kernel is not pinned.  Gradients flow into `tex` only.  Everything else nvdiffrast offers raises
NotImplementedError naming the reference call that would need it; street_crafter_amd.cubemap.sky_color does the whole of
SkyCubeMap.forward in one launch and is the faster call.
"""
from __future__ import annotations

import torch

from street_crafter_amd.cubemap import texture_cube

__all__ = ["texture"]


def texture(tex, uv, uv_da=None, mip_level_bias=None, mip=None, filter_mode="auto", boundary_mode="wrap",
            max_mip_level=None):
    """boundary_mode='cube' with filter_mode 'linear' or 'auto' and no mip arguments: tex [B,6,R,R,C] (a batch of 1
    broadcasts), uv [B,h,w,3] directions -> [B,h,w,C]."""
    if uv_da is not None or mip_level_bias is not None or mip is not None or max_mip_level is not None:
        raise NotImplementedError("nvdiffrast.torch.texture: mip-mapped sampling (uv_da / mip_level_bias / mip / "
                                  "max_mip_level) is not implemented; no call of the reference passes them")
    if boundary_mode != "cube":
        raise NotImplementedError(f"nvdiffrast.torch.texture: boundary_mode={boundary_mode!r} is not implemented; only "
                                  "latlong_to_cubemap (street_gaussian/models/sky_cubemap.py:188) samples a 2-D texture, "
                                  "and nothing calls it")
    if filter_mode not in ("linear", "auto"):
        raise NotImplementedError(f"nvdiffrast.torch.texture: filter_mode={filter_mode!r} is not implemented; the "
                                  "reference's cube calls (sky_cubemap.py:102,120,205) use 'linear'")
    if not isinstance(tex, torch.Tensor) or not isinstance(uv, torch.Tensor):
        raise TypeError("nvdiffrast.torch.texture: tex and uv must be torch tensors")
    if tex.dim() != 5 or tex.shape[1] != 6:
        raise ValueError(f"nvdiffrast.torch.texture: a cube texture must be [B,6,R,R,C], got {tuple(tex.shape)}")
    if uv.dim() != 4 or uv.shape[-1] != 3:
        raise ValueError(f"nvdiffrast.torch.texture: cube directions must be [B,h,w,3], got {tuple(uv.shape)}")
    B = uv.shape[0]
    if tex.shape[0] not in (1, B):
        raise ValueError(f"nvdiffrast.torch.texture: tex batch {tex.shape[0]} does not match uv batch {B}")
    if B == 1:
        return texture_cube(tex[0], uv[0])[None]
    return torch.stack([texture_cube(tex[b if tex.shape[0] > 1 else 0], uv[b]) for b in range(B)])


def _unsupported(name: str, where: str):
    def fn(*args, **kwargs):
        raise NotImplementedError(f"nvdiffrast.torch.{name} is not implemented on this platform; {where}")
    fn.__name__ = name
    return fn


_NOBODY = "the reference never calls it"
RasterizeCudaContext = _unsupported("RasterizeCudaContext", _NOBODY)
RasterizeGLContext = _unsupported("RasterizeGLContext", _NOBODY)
rasterize = _unsupported("rasterize", _NOBODY)
interpolate = _unsupported("interpolate", _NOBODY)
antialias = _unsupported("antialias", _NOBODY)
texture_construct_mip = _unsupported("texture_construct_mip", _NOBODY)
