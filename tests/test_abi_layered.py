"""CPU: every function include/aurppo.h declares with a ``size_t`` result is bound with ``restype = c_size_t`` (a workspace size
read as a C int is truncated above 2 GB and sign-extended by ctypes)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _size_t_functions():
    src = open(os.path.join(ROOT, "include", "aurppo.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\bsize_t\s+(aurppo_[a-z0-9_]+)\s*\(", src)))


def test_size_t_results_are_bound_as_size_t():
    import __graft_entry__ as g
    g.build()
    from aur_ppo_amd import _lib
    lib = _lib.load()
    names = _size_t_functions()
    assert "aurppo_mlp_wide_workspace_bytes" in names and "aurppo_head_ppo_workspace_bytes" in names and len(names) >= 8
    for name in names:
        assert getattr(lib, name).restype is ctypes.c_size_t, name


def test_head_workspace_plan_without_gpu():
    """aurppo_head_ppo_workspace_bytes is a host-side plan: statistics + one slab and one row of loss sums per workgroup; 0 outside K13's limits."""
    from aur_ppo_amd import _lib
    lib = _lib.load()
    for M, H, A in [(1, 32, 1), (257, 160, 6), (131072, 256, 6), (131072, 1024, 16)]:
        nb = lib.aurppo_head_ppo_workspace_bytes(M, H, A)
        assert nb >= ((A + 3) * H + 48) * 4 and nb < (1 << 27), (M, H, A, nb)
    assert lib.aurppo_head_ppo_workspace_bytes(131072, 256, 6) == lib.aurppo_head_ppo_workspace_bytes(2 * 131072, 256, 6)   # the grid is capped
    for M, H, A in [(0, 256, 6), (100, 100, 6), (100, 16, 6), (100, 1056, 6), (100, 256, 0), (100, 256, 17)]:
        assert lib.aurppo_head_ppo_workspace_bytes(M, H, A) == 0, (M, H, A)
    assert lib.aurppo_head_ppo_f32(*([None] * 7), 4, 256, 6, 1, None, None, 0, None, 0.2, 0.01, 0.5, 1, 1, None, None, None) == -1
    assert b"null pointer" in lib.aurppo_last_error()
