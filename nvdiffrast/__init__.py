"""Drop-in `nvdiffrast` package for StreetCrafter on MI355X: cube-map texture sampling only.

The reference imports `nvdiffrast.torch as dr` at module level (street_gaussian/models/sky_cubemap.py:6), and the
scene-graph model imports that module unconditionally (street_gaussian_model.py:21).  nvdiffrast itself is CUDA-only, so
without this package `street_gaussian/` does not import on a ROCm machine, whether or not a config enables the sky cube
map.  Putting this repository on PYTHONPATH makes `import nvdiffrast.torch` resolve to nvdiffrast/torch.py, whose
`texture(..., boundary_mode='cube')` is the HIP sampler of street_crafter_amd/cubemap.py; every other entry point of
nvdiffrast raises NotImplementedError.
"""
__version__ = "0.3.3+street_crafter_amd"
