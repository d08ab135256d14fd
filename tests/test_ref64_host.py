"""Host (no GPU): the fp64 reference of tests/ref64.py is right, its inputs keep clear of every branch point, and the bars of
tests/test_mlp_fp64_gpu.py have teeth -- a CPU emulation of the three-way bf16 split arithmetic (csrc/bf16x3.h) passes them
with its six products and fails them with any third-order product missing (DESIGN, parity section, lists every mutant)."""
import numpy as np
import pytest
import torch

from oracle import ppo_oracle as O
from tests import ref64 as R
from tests.util import load


# ------------------------------------------------------------------ the reference against the golden vectors
@pytest.mark.parametrize("name", ["cont_D64_A6", "disc_D4_A2", "cont_D5_A3_L3", "cont_D64_A6_H128_L3", "disc_D8_A4_H128_L2", "cont_D128_A6_H96_L1"])
def test_ref64_evaluate_and_gradients_match_the_reference_fixture(name):
    """evaluate.npz holds the real reference's log-prob, entropy, value and its autograd gradients of
    sum(w * logp) + 0.3 * sum(ent) + sum(val^2), w = linspace(0.5, 1.5, M).  ``run_step`` becomes exactly that with
    old_logp = logp (ratio 1), A_i = -M w_i without normalisation, ent_coef = -0.3 M, vf_coef = 2 M against returns of 0."""
    z = load("evaluate.npz")
    sd = {k[len(name) + 4:]: torch.from_numpy(z[k]) for k in z.files if k.startswith(f"{name}/sd/")}
    net = R.make_net(sd)
    D, A, hidden, layers, cont = R.net_shape(sd)
    assert (D, A, int(cont), layers, hidden) == tuple(int(x) for x in z[f"{name}/meta"])
    obs, act = torch.from_numpy(z[f"{name}/obs"]).double(), torch.from_numpy(z[f"{name}/act"]).double()
    M = obs.shape[0]
    rec = torch.zeros(M, 4, dtype=torch.float64)
    rec[:, 0] = torch.from_numpy(z[f"{name}/logp"]).double()
    rec[:, 1] = -M * torch.linspace(0.5, 1.5, M).double()
    out = R.run_step(net, obs, act, rec, 0.2, -0.3 * M, 2.0 * M, False, O.VLOSS_RETURNS, scales=True)
    # fp32 rounding level: the fixture is an fp32 computation (a few ulps of the terms' scale; 1e-6 as tests/test_oracle_golden.py)
    np.testing.assert_allclose(out["logp"].numpy(), z[f"{name}/logp"], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(out["ent"].numpy(), z[f"{name}/ent"], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(out["value"].numpy(), z[f"{name}/val"].reshape(-1), rtol=1e-6, atol=1e-6)
    # the gradients: the fixture is a plain fp32 computation, so it must lie as close to fp64 as plain fp32 does.  The yardstick is
    # this machine's fp32 run of the same step on the same metric; 4 x (the widest margin the kernels may ever get) because the
    # fixture formed its loss from other expressions, on another machine's BLAS
    y = R.run_step(R.make_net(sd, torch.float32), obs.float(), act.float(), rec.float(), 0.2, -0.3 * M, 2.0 * M, False, O.VLOSS_RETURNS)
    Y = max(R.grad_metrics(y["flat"], out).values())
    fix = torch.cat([torch.from_numpy(z[f"{name}/grad/{n}"]).reshape(-1) for n in out["names"]])
    m = R.grad_metrics(fix, out)
    assert max(m.values()) <= 4 * Y, (max(m, key=m.get), max(m.values()), Y)


def test_ref64_loss_matches_the_reference_fixture_and_the_oracle():
    """loss.npz: the real reference's scalars and the three gradient streams of its loss."""
    z = load("loss.npz")
    for name in z["names"]:
        T, N, norm_adv, clip_vloss, clip, ec, vc = z[f"{name}/meta"]
        if int(T) * int(N) == 2 and norm_adv:
            continue      # std of two points in fp32: tests/test_oracle_golden.py::test_loss_oracle_tiny_minibatch
        a = {k: torch.from_numpy(z[f"{name}/{k}"]).double().reshape(-1) for k in ("newlogp", "oldlogp", "adv", "newv", "oldv", "ret", "entropy")}
        lp, v, e = (a[k].clone().requires_grad_(True) for k in ("newlogp", "newv", "entropy"))
        rec = torch.stack([a["oldlogp"], a["adv"], a["ret"], a["oldv"]], 1)
        mode = O.VLOSS_CLIPPED if clip_vloss else O.VLOSS_OLDVALUES
        loss, sc, _ = R.loss_terms(lp, e, v, rec, clip, ec, vc, bool(norm_adv), mode)
        loss.backward()
        # the two "boundary" fixtures put samples EXACTLY on the clip edges (ratio == float32(1 +- clip), |v - v_old| == clip), where an
        # fp32 and an fp64 evaluation legitimately take different sides; they pin the oracle's tie rules (tests/test_oracle_golden.py).
        # Here their on-edge samples (and the clip fraction, which counts them) are left to that test; every other sample is held.
        d = R.branch_distances(a["newlogp"], a["newv"], rec, clip, bool(norm_adv), mode)
        off_edge = torch.stack([x.expand_as(a["newlogp"]) for x in d.values()]).min(0).values >= 1e-6
        cols = [1, 2, 3, 4, 5, 6]
        if "boundary" in str(name):
            assert 0 < int((~off_edge).sum()) < off_edge.numel() // 2
            cols = [1, 2, 3, 4, 5]
        else:
            assert bool(off_edge.all()), name
        m = off_edge.numpy()
        np.testing.assert_allclose(sc.numpy()[cols], z[f"{name}/scalars"][[c_ - 1 for c_ in cols]], rtol=2e-6, atol=2e-7, err_msg=name)
        np.testing.assert_allclose(lp.grad.numpy()[m], z[f"{name}/g_newlogp"][m], rtol=1e-5, atol=1e-9, err_msg=name)
        np.testing.assert_allclose(v.grad.numpy()[m], z[f"{name}/g_newv"][m], rtol=1e-5, atol=1e-9, err_msg=name)
        np.testing.assert_allclose(e.grad.numpy(), z[f"{name}/g_entropy"], rtol=1e-6, atol=0, err_msg=name)


@pytest.mark.parametrize("c", [c for c in R.K7_CASES + R.K7W_CASES if 2 <= c.M <= 1000], ids=R.case_id)
def test_ref64_loss_matches_the_oracle_on_margin_safe_inputs(c):
    """On inputs with no sample near a branch point the fp32 numpy oracle and the fp64 loss take the same branches: scalars and
    per-sample gradients agree at fp32 rounding level, with nothing excluded."""
    data = R.build_case(c)
    li = data["idx"].long()
    with torch.no_grad():
        _, lp, ent, v = data["net64"].evaluate(data["obs"][li].double(), data["act"][li].double() if c.cont else data["act"][li].long())
    lp32, ent32, v32 = (t.reshape(-1).float() for t in (lp, ent, v))          # what an exact forward pass would hand an fp32 loss
    rec = data["rec"][li]
    sc_o, glp_o, gv_o, ge_o = O.ppo_loss(lp32.numpy(), rec[:, 0].numpy(), rec[:, 1].numpy(), v32.numpy(), rec[:, 3].numpy(), rec[:, 2].numpy(),
                                         ent32.numpy(), R.HYPER["clip"], R.HYPER["ent_coef"], R.HYPER["vf_coef"], c.norm_adv, c.vmode)
    a, b, e = (t.double().requires_grad_(True) for t in (lp32, v32, ent32))
    loss, sc, _ = R.loss_terms(a, e, b, rec.double(), R.HYPER["clip"], R.HYPER["ent_coef"], R.HYPER["vf_coef"], c.norm_adv, c.vmode)
    loss.backward()
    assert sc_o[6] == np.float32(float(sc[6]))                                # the clip fraction: the same count
    np.testing.assert_allclose(sc_o, sc.numpy(), rtol=1e-5, atol=1e-6)
    s = float(a.grad.abs().max())
    np.testing.assert_allclose(glp_o, a.grad.numpy(), rtol=1e-5, atol=1e-6 * s)
    np.testing.assert_allclose(gv_o, b.grad.numpy(), rtol=1e-5, atol=1e-6 * float(b.grad.abs().max()))
    np.testing.assert_allclose(ge_o, e.grad.numpy(), rtol=1e-6)


# ------------------------------------------------------------------ the input builder: nothing near a branch point, nothing excluded
@pytest.mark.parametrize("c", R.K7_CASES + R.K7W_CASES + R.FWD_CASES, ids=R.case_id)
def test_builder_leaves_no_sample_near_a_branch_point(c):
    data = R.build_case(c)                     # asserts zero unsafe samples itself; checked again here from scratch
    li = data["idx"].long()
    with torch.no_grad():
        _, lp, _, v = data["net64"].evaluate(data["obs"][li].double(), data["act"][li].double() if c.cont else data["act"][li].long())
    d = R.branch_distances(lp, v.reshape(-1), data["rec"][li], R.HYPER["clip"], c.norm_adv, c.vmode)
    assert all(float(x.min()) >= R.BRANCH_EPS for x in d.values()), {k: float(x.min()) for k, x in d.items()}
    assert data["idx"].numel() == c.M and data["rec"].dtype == torch.float32
    if c.index == "repeat" and c.M > 2:
        assert torch.unique(data["idx"]).numel() < c.M
    if c.M >= 1000 and c.vmode == O.VLOSS_CLIPPED:      # the data still exercises both sides of every decision
        r = (lp - data["rec"][li][:, 0].double()).exp()
        assert float((r > 1.2).float().mean()) > 0.02 and float((r < 0.8).float().mean()) > 0.02
        assert 0.05 < float(((v.reshape(-1) - data["rec"][li][:, 3].double()).abs() > 0.2).float().mean()) < 0.95


@pytest.mark.parametrize("A,N", [(2, 77), (5, 33), (16, 4096)])
def test_safe_uniform_leaves_no_draw_near_a_cdf_edge(A, N):
    rs = np.random.RandomState(A)
    net = R.make_net(R.make_policy_sd(64, 2, 8, A, False, rs))
    obs, u = R.make_obs(N, 8, "normal", rs), torch.from_numpy(rs.random_sample(N).astype(np.float32))
    R.safe_uniform(net, obs, u)
    ref = R.act_reference(net, obs, u)
    assert float((u.double()[:, None] - ref["cdf"][:, :-1]).abs().min()) >= R.BRANCH_EPS and bool(((u >= 0) & (u < 1)).all())


# ------------------------------------------------------------------ the bars have teeth
@pytest.fixture
def one_thread():
    """The yardstick is an fp32 matrix product on the CPU: one thread fixes its summation order, so the ratios printed here are the
    same on every machine of this kind."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def _drop(prods):
    return R.SIX - set(prods)


def _teeth_case(M):
    c = R._mk("k7", 64, 2, 64, 6, True, M, True, 1)
    data = R.build_case(c)
    data["ref"] = R.reference_step(c, data)
    Y, Ys, _ = R.yardstick_step(c, data, "cpu")
    return c, data, Y, Ys


def _emulated_ratio(c, data, Y, prods_of):
    li = data["idx"].long()
    net = R.make_emulated_net(data["sd"], prods_of)
    got = R.run_step(net, data["obs"][li], data["act"][li], data["rec"][li], R.HYPER["clip"], R.HYPER["ent_coef"], R.HYPER["vf_coef"],
                     c.norm_adv, c.vmode)
    gm = R.grad_metrics(got["flat"], data["ref"])
    return max(gm.values()) / Y, got


# single-role mutants: (layer, role) of the 2 x 64 policy; layer 0 first, 1 hidden, 2 head.  The head's forward is the one the
# gradient bar cannot see (DESIGN): the per-sample forward check below is what rejects it.
GRAD_ROLES = [(0, "fwd"), (1, "fwd"), (1, "dx"), (2, "dx"), (0, "dw"), (1, "dw"), (2, "dw")]


@pytest.mark.parametrize("M", [1000, 20000])
def test_gradient_bar_passes_six_products_and_rejects_every_mutant(M, one_thread):
    c, data, Y, _ = _teeth_case(M)
    six, _ = _emulated_ratio(c, data, Y, lambda l, r: R.SIX)
    print(f"\nM={M} Y={Y:.3e}  six products: {six:.2f} x Y")
    assert six <= R.MARGIN, six
    for p in R.THIRD_ORDER:                      # one third-order product missing from EVERY product of the step
        ratio, _ = _emulated_ratio(c, data, Y, lambda l, r: _drop([p]))
        print(f"M={M} a{p[0]}*b{p[1]} dropped everywhere: {ratio:.1f} x Y")
        assert ratio > R.MARGIN, (p, ratio)
    for role in GRAD_ROLES:                      # all three missing from a single role
        ratio, _ = _emulated_ratio(c, data, Y, lambda l, r: _drop(R.THIRD_ORDER) if (l, r) == role else R.SIX)
        print(f"M={M} third order dropped in layer {role[0]} {role[1]}: {ratio:.1f} x Y")
        assert ratio > R.MARGIN, (role, ratio)
    # recorded, not asserted (DESIGN's table marks what no check rejects): just a1*b1 missing from one role; the head's forward
    for role in GRAD_ROLES + [(2, "fwd")]:
        r1, _ = _emulated_ratio(c, data, Y, lambda l, r: _drop([(1, 1)]) if (l, r) == role else R.SIX)
        r3, _ = _emulated_ratio(c, data, Y, lambda l, r: _drop(R.THIRD_ORDER) if (l, r) == role else R.SIX)
        print(f"M={M} layer {role[0]} {role[1]}: a1*b1 dropped {r1:.1f} x Y, third order dropped {r3:.1f} x Y (gradient bar)")


def test_per_sample_forward_bar_rejects_a_wrong_head_product(one_thread):
    """Minibatches of one sample expose log-prob, entropy and value (tests/test_mlp_fp64_gpu.py): on them the head's forward
    product with its third-order terms missing is in plain sight, where the gradient bar sees 1.5 x Y at most."""
    c = R._mk("k7", 64, 2, 64, 6, True, 64, False, 0)
    data = R.build_case(c)
    li = data["idx"].long()
    obs, act, rec = data["obs"][li], data["act"][li], data["rec"][li]
    ref = R.run_step(data["net64"], obs.double(), act.double(), rec.double(), 0.2, 0.01, 1.0, False, 0, scales=True)

    def fwd(net):
        with torch.no_grad():
            _, lp, ent, v = net.evaluate(obs, act)
        return R.forward_metrics(lp, ent, v, ref)
    y = fwd(R.make_net(data["sd"], torch.float32))
    Y = max(y.values())
    six = fwd(R.make_emulated_net(data["sd"], lambda l, r: R.SIX))
    print(f"\nforward Y={Y:.3e} (fp32 torch {y}); six products {six}")
    assert max(six.values()) <= R.MARGIN * Y
    for prods, what in ((_drop(R.THIRD_ORDER), "third order"), (_drop([(1, 1)]), "a1*b1"), (_drop([(0, 2)]), "a0*b2"), (_drop([(2, 0)]), "a2*b0")):
        for layer in (2, 1, 0):
            m = fwd(R.make_emulated_net(data["sd"], lambda l, r: prods if (l, r) == (layer, "fwd") else R.SIX))
            print(f"layer {layer} forward, {what} dropped: " + ", ".join(f"{k} {v / Y:.1f} x Y" for k, v in m.items()))
            assert max(m["logp"], m["value"]) > R.MARGIN * Y, (layer, what, m)


# ------------------------------------------------------------------ where the class margins come from
@pytest.mark.parametrize("M,n_seeds", [(1, 30), (2, 30), (31, 30), (65, 30), (1000, 15)])
def test_a_second_correct_fp32_formulation_meets_the_bars_of_every_class(M, n_seeds, one_thread):
    """``make_alternative_fp32_net`` is correct fp32 arithmetic (exact six-product matrix products; the kernels' tanh, log-prob and
    softmax formulas where they differ from torch's).  Judged against Y like a kernel, over many seeds, it shows what a bar may ask of
    ANY correct implementation: at M >= 31 every gradient tensor stays under MARGIN x Y; at fewer samples, and for the nine scalars at
    every M, Y is the rounding of a handful of numbers and two correct computations lie up to 39 x (gradients, 237 draws at M = 1, 2)
    and 11.5 x (scalars, 597 draws) apart -- hence MARGIN_TINY_M and MARGIN_SCALARS (DESIGN, parity section, has the full table)."""
    worst_g = worst_s = 0.0
    for seed in range(n_seeds):
        for cont, vmode, norm in ((True, 1, M > 1), (False, 0, False)):
            c = R._mk("k7", 64, 2, 16, 6, cont, M, norm, vmode)._replace(seed=1000 * M + seed)
            data = R.build_case(c)
            data["ref"] = R.reference_step(c, data)
            Y, Ys, _ = R.yardstick_step(c, data, "cpu")
            li = data["idx"].long()
            got = R.run_step(R.make_alternative_fp32_net(data["sd"]), data["obs"][li], data["act"][li] if cont else data["act"][li].long(),
                             data["rec"][li], R.HYPER["clip"], R.HYPER["ent_coef"], R.HYPER["vf_coef"], c.norm_adv, c.vmode)
            _, _, rg, rs = R.check_step(c, got["scalars"], got["flat"], data["ref"], Y, Ys, f"alternative fp32, seed {seed}")
            worst_g, worst_s = max(worst_g, rg), max(worst_s, rs)
    print(f"\nM={M}: worst gradient ratio {worst_g:.2f} (margin {R.grad_margin(M):g}), worst scalar ratio {worst_s:.2f} (margin {R.MARGIN_SCALARS:g})")
