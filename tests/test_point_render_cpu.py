"""No-GPU checks of the LiDAR point render (csrc/point_raster.hip, street_crafter_amd/point_render.py and the drop-in
`diff_point_rasterization` package): the two entry points are declared, exported and in the ctypes table, bad
arguments are refused before any launch, and the drop-in imports, has the reference's settings and refuses CPU
tensors."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sc_point_project", "sc_point_rasterize_fwd")


@pytest.fixture(scope="module")
def lib():
    from street_crafter_amd import build
    build.build()
    from street_crafter_amd import _lib
    return _lib.load()


def test_point_entry_points_declared_exported_and_bound(lib):
    from street_crafter_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "street_crafter_amd.h")).read(), flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(rf"\bint\s+{name}\s*\(", src), name
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name
    assert "point_raster.hip" in __import__("street_crafter_amd.build", fromlist=["SOURCES"]).SOURCES


def _project(lib, N=4, occ=1.0, ptr=None, mode=0, radius_in=None, width=64, height=48, opac=None, focal=100.0,
             scale=0.01):
    return lib.sc_point_project(ptr, ptr, opac, occ, radius_in, N, ptr, 100.0, 100.0, 32.0, 24.0, focal, width, height,
                                1.0, 100.0, mode, scale, 1.0, ptr, ptr, ptr, ptr, None)


def _raster(lib, N=4, max_hit=10, ptr=None, width=64, height=48, tw=4, th=3, strides=(4, 1, 4), n_isects=8):
    return lib.sc_point_rasterize_fwd(ptr, N, width, height, tw, th, ptr, ptr, n_isects, max_hit, None, ptr,
                                      strides[0], strides[1], ptr, strides[2], None, None)


def test_point_entry_points_refuse_bad_arguments_before_launching(lib):
    # a non-null pointer that is never dereferenced: every call below is refused on the host
    fake = 0x10000
    assert _project(lib, N=4) == -1                                   # null pointers
    assert _project(lib, N=-1, ptr=fake) == -1                        # N < 0
    assert _project(lib, occ=0.0, ptr=fake) == -1                     # occ outside (0, 1]
    assert _project(lib, occ=1.5, ptr=fake) == -1
    assert _project(lib, occ=float("nan"), ptr=fake) == -1
    assert _project(lib, mode=4, ptr=fake) == -1                      # unknown radius mode
    assert _project(lib, mode=2, ptr=fake) == -1                      # knn mode without distances
    assert _project(lib, mode=3, ptr=fake) == -1                      # per-point radius without the array
    assert _project(lib, width=0, ptr=fake) == -1
    assert _project(lib, focal=0.0, ptr=fake) == -1
    assert _project(lib, scale=-1.0, ptr=fake) == -1
    assert _project(lib, N=0) == 0                                    # nothing to do: no launch, no pointer read
    assert _raster(lib) == -1                                         # null pointers
    assert _raster(lib, N=-1, ptr=fake) == -1
    assert _raster(lib, max_hit=0, ptr=fake) == -1                    # max_hit < 1
    assert _raster(lib, tw=3, ptr=fake) == -1                         # not the 16-pixel tile grid of the image
    assert _raster(lib, strides=(0, 1, 4), ptr=fake) == -1
    assert _raster(lib, strides=(4, 1, 0), ptr=fake) == -1
    assert _raster(lib, n_isects=-1, ptr=fake) == -1
    assert _raster(lib, ptr=fake + 4) == -1                           # records not 16-B aligned


def test_drop_in_package_settings_and_cpu_refusal():
    import diff_point_rasterization as dpr
    # render_utils.py:150-164, in that order
    assert dpr.PointRasterizationSettings._fields == (
        "image_height", "image_width", "tanfovx", "tanfovy", "bg", "scale_modifier", "viewmatrix", "projmatrix",
        "sh_degree", "max_hit", "campos", "prefiltered", "debug")
    s = dpr.PointRasterizationSettings(image_height=48, image_width=64, tanfovx=0.32, tanfovy=0.24,
                                       bg=torch.zeros(3), scale_modifier=1.0, viewmatrix=torch.eye(4),
                                       projmatrix=torch.eye(4), sh_degree=0, max_hit=10, campos=torch.zeros(3),
                                       prefiltered=False, debug=False)
    r = dpr.PointRasterizer(raster_settings=s)
    assert isinstance(r, torch.nn.Module)
    n = 8
    with pytest.raises(RuntimeError, match="HIP device"):
        r(means3D=torch.zeros(n, 3), means2D=torch.zeros(n, 3), colors_precomp=torch.zeros(n, 3),
          opacities=torch.ones(n, 1), radius=torch.ones(n, 1))
    with pytest.raises(NotImplementedError):
        r(means3D=torch.zeros(n, 3), means2D=torch.zeros(n, 3), colors_precomp=None, opacities=torch.ones(n, 1),
          radius=torch.ones(n, 1))
    with pytest.raises(NotImplementedError):
        dpr.PointRasterizer(s._replace(sh_degree=3))(means3D=torch.zeros(n, 3), means2D=None,
                                                     colors_precomp=torch.zeros(n, 3), opacities=torch.ones(n, 1),
                                                     radius=torch.ones(n, 1))


def _projection_3dgs(znear, zfar, fovx, fovy):
    """3DGS getProjectionMatrix (column form), centred principal point."""
    t, r = np.tan(fovy / 2) * znear, np.tan(fovx / 2) * znear
    P = np.zeros((4, 4))
    P[0, 0], P[1, 1] = 2 * znear / (2 * r), 2 * znear / (2 * t)
    P[3, 2], P[2, 2], P[2, 3] = 1.0, zfar / (zfar - znear), -(zfar * znear) / (zfar - znear)
    return P


def test_drop_in_camera_is_read_back_from_the_settings():
    import diff_point_rasterization as dpr
    H, W, fx, fy = 48, 64, 80.0, 70.0
    fovx, fovy = 2 * np.arctan(W / (2 * fx)), 2 * np.arctan(H / (2 * fy))
    w2c = np.eye(4)
    w2c[:3, :3] = np.array([[0, -1, 0], [0, 0, -1], [1, 0, 0]], float)
    w2c[:3, 3] = [0.5, -1.0, 3.0]
    V = w2c.T                                                          # row-vector form, as 3DGS stores it
    F = V @ _projection_3dgs(1.0, 100.0, fovx, fovy).T
    s = dpr.PointRasterizationSettings(H, W, np.tan(fovx / 2), np.tan(fovy / 2), None, 1.0, torch.from_numpy(V),
                                       torch.from_numpy(F), 0, 10, None, False, False)
    m, gfx, gfy, gcx, gcy, zn, zf, focal_r = dpr.camera_from_settings(s)
    np.testing.assert_allclose(m, w2c, atol=1e-12)
    np.testing.assert_allclose([gfx, gfy, gcx, gcy, zn, zf, focal_r], [fx, fy, W / 2, H / 2, 1.0, 100.0, fx], rtol=1e-9)
    bad = F.copy()
    bad[:, 3] = 0.0                                                    # an orthographic-like w: not a pinhole
    with pytest.raises(NotImplementedError):
        dpr.camera_from_settings(s._replace(projmatrix=torch.from_numpy(bad)))


def test_point_render_refuses_cpu_tensors_and_bad_parameters():
    from street_crafter_amd.point_render import render_points_hip
    pts, feat = torch.zeros(4, 3), torch.ones(4, 5)
    with pytest.raises(RuntimeError, match="HIP device"):
        render_points_hip(np.eye(4), np.eye(3), pts, feat, 8, 8)
    with pytest.raises(ValueError):
        render_points_hip(np.eye(4), np.eye(3), pts, feat, 8, 8, occ=1.5)
    with pytest.raises(ValueError):
        render_points_hip(np.eye(4), np.eye(3), pts, feat, 8, 8, max_hit=0)


def test_setup_installs_the_drop_in_package():
    src = open(os.path.join(ROOT, "setup.py")).read()
    inc = re.search(r"find_packages\(include=\[(.*?)\]\)", src, flags=re.S).group(1)
    assert '"diff_point_rasterization"' in inc


def test_new_modules_never_import_oracle():
    for rel in ("street_crafter_amd/point_render.py", "diff_point_rasterization/__init__.py"):
        src = open(os.path.join(ROOT, rel)).read()
        assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), rel
        assert "oracle" not in re.findall(r"^\s*(?:from|import)\s+([\w.]+)", src, flags=re.M), rel
