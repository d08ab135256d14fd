"""CPU: K13's workspace plan and argument validation need no device.  (That every ``size_t`` result is bound as ``c_size_t``
is part of tests/test_abi_signatures.py.)"""


def test_head_workspace_plan_without_gpu():
    """aurppo_head_ppo_workspace_bytes is a host-side plan: statistics + one slab and one row of loss sums per workgroup; 0 outside K13's limits."""
    import __graft_entry__ as g
    g.build()
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
