"""backsub_mcc_kernel / _batch / _marg (csrc/k_reproj.hip) with the short dependent chain: the tangent offsets per factor (Visual::fac_t)
instead of the hop through the camera-pose id, the pose step staged in LDS, and — in the compact layout — everything a lane's first two
factors need in either pass asked for at once.  The arithmetic is the parent's, so every check is the one tests/test_gpu_band.py makes for
two assemblies of one system and for the oracle: per-iteration cost rtol 1e-10, step norm rtol 1e-6, final cost 1e-9 of the oracle's,
values 1e-6; a batch against its lone solves as test_no_c_rows_lone_and_batched_steps_on_the_same_contexts (1e-10, 1e-7).
Lanes with no, one, two and three factors; the three row formats (compact, full without C rows, full with C rows); the factor-per-lane
workgroups of constant landmarks; held blocks (an offset of -1); the gather from memory above the staging limit; the table's upkeep."""
import functools

import numpy as np
import pytest

from beam_slam_amd import capi, synthetic

pytestmark = pytest.mark.gpu


def _n_reproj(pr):
    return sum(int(t[0].shape[0]) for t in pr.factors[capi.F_REPROJ])


@functools.lru_cache(maxsize=None)
def _window(kind):
    if kind == "short":          # tracks of 2 - 9 views: lanes with no factor and with one; every landmark a band landmark
        return synthetic.vio_window(n_kf=12, n_lm=300, seed=81, track_min=2, track_max=9)
    if kind == "long":           # tracks of up to 20 views: two factors per lane from 9 views, a third from 17; the long ones keep pair entries and C rows
        return synthetic.vio_window(n_kf=40, n_lm=900, seed=82, track_min=2, track_max=20)
    if kind == "held":
        pr = synthetic.vio_window(n_kf=24, n_lm=600, seed=83, track_min=2, track_max=13)
        for b in pr.meta["lm_blocks"][::9]:            # constant landmarks: the factor-per-lane workgroups, the full layout
            pr.is_const[int(b)] = 1
        for b in pr.meta["kf_blocks"][5][:2]:          # q and p held: fac_t = (-1, -1)
            pr.is_const[int(b)] = 1
        pr.is_const[int(pr.meta["kf_blocks"][11][1])] = 1   # p alone held: tq >= 0, tp < 0
        return pr
    if kind == "wide":           # 280 key frames x 15 = 4 200 reduced dimensions: above the 4 096 the staging takes
        return synthetic.vio_window(n_kf=280, n_lm=600, seed=84, track_min=2, track_max=9)
    raise ValueError(kind)


def _options(solver, iters):
    o = solver.options_vio()
    o.max_num_iterations = iters
    o.max_solver_time_in_seconds = 0.0
    return o


@functools.lru_cache(maxsize=None)
def _oracle(kind, iters):
    from oracle import Oracle
    o = Oracle()
    _window(kind).load(o)
    s = o.solve(_options(o, iters))
    return s.final_cost, o.get_blocks()


def _run(pr, gpu_solver_cls, iters):
    g = gpu_solver_cls(0)
    pr.load(g)
    s = g.solve(_options(g, iters))
    return s, [(i.cost, i.step_norm) for i in g.iterations()], g.get_blocks(), g.reproj_jacobian_bytes()


def _against_oracle(tag, kind, iters, run):
    s, it, x, _ = run
    cost_o, x_o = _oracle(kind, iters)
    gap_c, gap_x = abs(s.final_cost - cost_o) / cost_o, float(np.abs(x - x_o).max())
    print(f"{tag}: final cost gap to the oracle {gap_c:.3e}, values gap {gap_x:.3e}")
    assert gap_c <= 1e-9
    assert gap_x < 1e-6


def _same_trajectory(tag, a, b):
    (_, it0, x0, _), (_, it1, x1, _) = a, b
    assert len(it0) == len(it1)
    c0, c1 = np.array([i[0] for i in it0]), np.array([i[0] for i in it1])
    n0, n1 = np.array([i[1] for i in it0]), np.array([i[1] for i in it1])
    print(f"{tag}: cost gap {float(np.max(np.abs(c0 - c1) / np.abs(c0))):.3e}, step norm gap {float(np.max(np.abs(n0 - n1) / np.maximum(np.abs(n0), 1e-300))):.3e}, "
          f"values gap {float(np.abs(x0 - x1).max()):.3e}")
    assert np.allclose(c0, c1, rtol=1e-10, atol=0.0)
    assert np.allclose(n0, n1, rtol=1e-6, atol=1e-12)
    assert np.abs(x0 - x1).max() < 1e-6


def test_compact_and_full_layouts(gpu_solver_cls, monkeypatch):
    """the three row formats of one window: compact pose part without C rows (the library's choice), the full pose part without C rows
    (BSGPU_COMPACT_J=0), the full pose part with C rows (BSGPU_NO_CR=0) — each against the oracle, and the same trajectory"""
    monkeypatch.setenv("BSGPU_PAIRS_BAND", "1")
    pr, n = _window("short"), _n_reproj(_window("short"))
    compact = _run(pr, gpu_solver_cls, 6)
    monkeypatch.setenv("BSGPU_COMPACT_J", "0")
    full = _run(pr, gpu_solver_cls, 6)
    monkeypatch.delenv("BSGPU_COMPACT_J")
    monkeypatch.setenv("BSGPU_NO_CR", "0")
    with_cr = _run(pr, gpu_solver_cls, 6)
    assert full[3] - compact[3] == 48 * n and with_cr[3] == full[3], (compact[3], full[3], with_cr[3], n)   # (the layouts were the ones meant)
    for tag, run in (("compact", compact), ("full", full), ("C rows", with_cr)):
        _against_oracle(tag, "short", 6, run)
    _same_trajectory("compact / full", compact, full)
    _same_trajectory("compact / C rows", compact, with_cr)


def test_long_tracks_reload_in_the_second_pass(gpu_solver_cls, monkeypatch):
    """tracks of 17 - 20 views give a lane a third factor, which loads again in the second pass; the long tracks keep pair entries and C rows"""
    monkeypatch.setenv("BSGPU_PAIRS_BAND", "1")
    pr = _window("long")
    idx = np.concatenate([t[0] for t in pr.factors[capi.F_REPROJ]])
    assert np.bincount(idx[:, 2]).max() >= 17
    _against_oracle("long tracks", "long", 6, _run(pr, gpu_solver_cls, 6))


def test_held_and_constant_blocks(gpu_solver_cls, monkeypatch):
    """constant landmarks (a factor per lane), a key frame held whole and a key frame whose position alone is held"""
    monkeypatch.setenv("BSGPU_PAIRS_BAND", "1")
    pr = _window("held")
    g = gpu_solver_cls(0)
    pr.load(g)
    ft, joined = g.backsub_tangent_table(_n_reproj(pr))
    assert np.array_equal(ft, joined)
    assert np.any((ft[:, 0] == -1) & (ft[:, 1] == -1)) and np.any((ft[:, 0] >= 0) & (ft[:, 1] == -1)) and np.any((ft[:, 0] >= 0) & (ft[:, 1] >= 0))
    _against_oracle("held and constant", "held", 6, _run(pr, gpu_solver_cls, 6))


def test_above_the_staging_limit(gpu_solver_cls, monkeypatch):
    """a reduced system of more than 4 096 dimensions: the pose step is gathered from memory"""
    monkeypatch.setenv("BSGPU_PAIRS_BAND", "1")
    pr = _window("wide")
    g = gpu_solver_cls(0)
    pr.load(g)
    g.finalize()
    assert g.num_parameters_tangent() - 3 * 600 > 4096
    _against_oracle("above the limit", "wide", 2, _run(pr, gpu_solver_cls, 2))


def test_batch_equals_lone_solves(gpu_solver_cls, monkeypatch):
    """the three windows in one solve_batch (one launch: staged, from its largest window; three row formats side by side) against their lone solves"""
    monkeypatch.setenv("BSGPU_PAIRS_BAND", "1")
    cases = [_window("short"), _window("long"), _window("held")]

    def fresh():
        out = []
        for pr in cases:
            g = gpu_solver_cls(0); pr.load(g); out.append(g)
        return out
    lone = fresh()
    opt = _options(lone[0], 4)
    ref = [(g.solve(opt).final_cost, g.get_blocks()) for g in lone]
    gs = fresh()
    sums = gpu_solver_cls.solve_batch(gs, opt)
    for k, (g, s, (c0, x0)) in enumerate(zip(gs, sums, ref)):
        gap_c, gap_x = abs(s.final_cost - c0) / c0, float(np.abs(g.get_blocks() - x0).max())
        print(f"window {k}: batch against lone, final cost gap {gap_c:.3e}, values gap {gap_x:.3e}")
        assert gap_c <= 1e-10 and gap_x < 1e-7


def _tables_agree(g, n):
    ft, joined = g.backsub_tangent_table(n)
    assert np.array_equal(ft, joined)
    return ft


def test_table_follows_every_flattening(gpu_solver_cls, monkeypatch):
    """fac_t = (cp_tq, cp_tp)[cam_pose] after a device flattening, equal to the host flattening's; after a sliding-window cycle through
    bsgpu_sync_factors_indirect; after a block's constness is toggled and the context finalized again — and each time the solve is a fresh context's"""
    from test_sync_tables import SlidingWindow, _describe
    monkeypatch.setenv("BSGPU_PAIRS_BAND", "1")
    pr = _window("held")
    n = _n_reproj(pr)
    monkeypatch.setenv("BSGPU_FLATTEN", "host")
    h = gpu_solver_cls(0); pr.load(h)
    ft_host = _tables_agree(h, n)
    monkeypatch.setenv("BSGPU_FLATTEN", "device")
    d = gpu_solver_cls(0); pr.load(d)
    ft_dev = _tables_agree(d, n)
    assert np.array_equal(ft_dev, ft_host) and ft_dev.min() == -1 and ft_dev.max() > 0
    opt = _options(d, 4)
    sh, sd = h.solve(opt), d.solve(opt)
    assert abs(sh.final_cost - sd.final_cost) <= 1e-10 * sh.final_cost and np.abs(h.get_blocks() - d.get_blocks()).max() < 1e-7
    # constness toggled on the SAME context: the held key frame is released, another one is held
    kf = pr.meta["kf_blocks"]
    saved = list(pr.is_const)
    try:
        for b in kf[5][:2]:
            pr.is_const[int(b)] = 0
        for b in kf[8][:2]:
            pr.is_const[int(b)] = 1
        pr.load(d)
        ft_toggled = _tables_agree(d, n)
        assert not np.array_equal(ft_toggled, ft_dev)
        f = gpu_solver_cls(0); pr.load(f)
        assert np.array_equal(_tables_agree(f, n), ft_toggled)
        s0, s1 = d.solve(opt), f.solve(opt)
        assert abs(s0.final_cost - s1.final_cost) <= 1e-10 * s1.final_cost and np.abs(d.get_blocks() - f.get_blocks()).max() < 1e-7
    finally:
        pr.is_const[:] = saved
    # a window that slides, handed over as change lists (the device-resident table, device flattening)
    w = SlidingWindow(np.random.default_rng(29), 7, 30, 40)
    a = gpu_solver_cls(0)
    for cyc in range(3):
        if cyc:
            w.drop_oldest(free_landmarks=cyc % 2 == 0)
            w.add_keyframe()
        blocks = w.blocks()
        b = gpu_solver_cls(0)
        _describe(w, a, blocks, True, cyc == 0)
        _describe(w, b, blocks, False, False)
        m = w.idx.shape[0]
        assert np.array_equal(_tables_agree(a, m), _tables_agree(b, m)), cyc
        sa, sb = a.solve(), b.solve()
        assert sa.termination_type == sb.termination_type and abs(sa.final_cost - sb.final_cost) <= 1e-8 * sb.final_cost, cyc   # (as test_sync_tables._cycles)
