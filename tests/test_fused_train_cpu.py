"""No-GPU checks of the fused training route of `rasterization()`: the switch (off by default, SC_FUSED_TRAIN,
set_fused_training) and the argument validation of sc_projection_sh_bwd through the ctypes table -- everything here is
rejected or answered before any launch, so nothing touches a device."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SC_OK, SC_EINVAL = 0, -1


@pytest.fixture(scope="module")
def lib():
    from street_crafter_amd import build
    build.build()
    from street_crafter_amd import _lib
    return _lib.load()


def test_fused_training_is_off_by_default_and_on_from_the_environment():
    code = ("import sys; sys.path.insert(0, %r); from street_crafter_amd import rendering as R; "
            "print(R._SWITCH.fused_train)" % ROOT)
    env = dict(os.environ)
    env.pop("SC_FUSED_TRAIN", None)

    def run(**extra):
        return subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, check=True,
                              env=dict(env, **extra)).stdout.split()

    assert run() == ["False"]
    assert run(SC_FUSED_TRAIN="1") == ["True"]
    assert run(SC_FUSED_TRAIN="0") == ["False"]
    assert run(SC_FUSED_TRAIN="") == ["False"]          # an empty variable is the default, as for the other switches


def test_set_fused_training_returns_the_previous_value():
    from street_crafter_amd import rendering
    first = rendering.set_fused_training(True)
    try:
        assert rendering._SWITCH.fused_train is True
        assert rendering.set_fused_training(False) is True and rendering._SWITCH.fused_train is False
        assert rendering.set_fused_training(1) is False and rendering._SWITCH.fused_train is True
    finally:
        rendering.set_fused_training(first)
    assert rendering._SWITCH.fused_train is first
    assert "SC_FUSED_TRAIN" in rendering._Switches.__doc__ and "fused_train" in rendering._Switches.__slots__


def _bwd(lib, C=1, N=8, K=4, deg=1, width=64, height=64, ptr=None):
    """sc_projection_sh_bwd with every pointer `ptr` (None = NULL; nothing is launched for the arguments used here)."""
    return lib.sc_projection_sh_bwd(*([ptr] * 8), C, N, K, deg, width, height, 0.3, 1, *([ptr] * 12), None)


def test_projection_sh_bwd_argument_validation_without_gpu(lib):
    assert _bwd(lib, deg=5, K=36) == SC_EINVAL                  # degree > 4
    assert _bwd(lib, deg=-1) == SC_EINVAL
    assert _bwd(lib, deg=1, K=3) == SC_EINVAL                   # K < (deg + 1)^2
    assert _bwd(lib, deg=3, K=15) == SC_EINVAL
    assert _bwd(lib, N=-1) == SC_EINVAL                         # negative sizes
    assert _bwd(lib, C=-1) == SC_EINVAL
    assert _bwd(lib, width=0) == SC_EINVAL and _bwd(lib, height=0) == SC_EINVAL
    assert _bwd(lib) == SC_EINVAL                               # NULL required pointers
    assert _bwd(lib, N=0) == SC_OK                              # nothing to do: no pointer is looked at
    assert _bwd(lib, N=0, deg=5, K=36) == SC_EINVAL             # ... but the degree still is
    # each required pointer on its own: NULL in one place, a (never dereferenced) non-NULL value everywhere else
    req = list(range(8)) + [16, 17, 18, 20, 21, 22]             # leaves, cameras, radii, conics, the upstream but v_depths
    # (no gradient is asked for, so even the complete argument list returns before a launch)
    full = [0x1000] * 8 + [1, 8, 4, 1, 64, 64, 0.3, 1] + [0x1000] * 7 + [None] * 5 + [None]
    assert lib.sc_projection_sh_bwd(*full) == SC_OK
    for i in req:
        args = list(full)
        args[i] = None
        assert lib.sc_projection_sh_bwd(*args) == SC_EINVAL, i
    args = list(full)
    args[19] = None                                             # v_depths is optional
    assert lib.sc_projection_sh_bwd(*args) == SC_OK


def test_signature_table_matches_the_header():
    import re
    from street_crafter_amd import _lib
    src = open(os.path.join(ROOT, "include", "street_crafter_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"int\s+sc_projection_sh_bwd\s*\((.*?)\)\s*;", src, flags=re.S)
    assert m, "sc_projection_sh_bwd is not declared"
    params = [a.strip() for a in m.group(1).split(",")]
    res, args = _lib.SIGNATURES["sc_projection_sh_bwd"]
    assert len(params) == len(args) == 29
    import ctypes
    for decl, ct in zip(params, args):
        want = ctypes.c_void_p if ("*" in decl or "sc_stream_t" in decl) else (ctypes.c_float if decl.startswith("float") else ctypes.c_int)
        assert ct is want, (decl, ct)
