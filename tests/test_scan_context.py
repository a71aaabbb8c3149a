"""bsgpu_scan_context_describe / bsgpu_scan_context_match on the CPU: beam_slam_amd/csrc/scan_context.h (through
tests/plan/test_scan_context.cpp, the kernels' arithmetic and order of addition on one core) against the NumPy restatement of the
contract (tests/scan_context_ref.py: arctan2, numpy.maximum.at, plain mean / norm, brute force over shifts).

Scenes (scan_context_ref.VIEWS): 4 000 rays of a 16-beam revolution from inside a box room with round pillars — place A (20 x 14 x 5 m,
three pillars) from (1, 0.5), A revisited from (1.3, 0.3) at 93 degrees yaw, A from (-6, 3) at 200 degrees, place B (34 x 8 x 3 m, two
pillars), place C (an empty 60 x 50 x 9 m hall); lidar_height 2, max_radius 40.  Measured on these scenes: A against A revisited 0.087 at
shift 15 (93 / 6 = 15.5), against the other three 0.82, 0.74, 0.96; see test_match_against_restatement.

Before anything is compared every case asserts that its input can be compared (`comparable`): every point at least 1e-9 of a bin away
from a ring or sector boundary; the gaps between best and second-best alignment norm, best and second-best shift distance, best and
second-best candidate, K-th and (K + 1)-th ring-key distance, and between every best distance and dist_thres above 1e-9.

Cases without a revisit (MATCH_CASES "none_*") check the -1 decision for finite distances against the restatement.

Accuracy criterion: descriptors, n_binned, best_cand, best_shift, every shift and the pre-selected sets equal; keys, distances and yaw
within 8 x the restatement's own difference under a reversed summation order (not below 2^-52 of the quantity's largest magnitude).
"""
import os
import subprocess

import numpy as np
import pytest

import scan_context_ref as ref
from scan_context_ref import bin_command, describe_command, match_command  # noqa: F401  (the GPU tests take them from here)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "plan", "test_scan_context.cpp")
INC = os.path.join(ROOT, "beam_slam_amd", "csrc")
NB = ref.RINGS * ref.SECTORS


def run_program(exe, commands, tmp_path):
    """commands: arrays of doubles -> per command the program's output line as a token list."""
    path = tmp_path / "commands.bin"
    np.concatenate(commands).astype(np.float64).tofile(str(path))
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and f"DONE {len(commands)}" in r.stdout and not r.stderr, r.stdout[-2000:] + r.stderr[-4000:]
    rows = [ln.split() for ln in r.stdout.splitlines() if not ln.startswith("DONE")]
    assert [int(t[1]) for t in rows] == list(range(len(commands)))
    return rows


def parse_describe(tok, A):
    v = tok[2:]
    f = lambda a, b: np.array([float(x) for x in v[a:b]])
    o = A
    return dict(n_binned=np.array([int(x) for x in v[:A]], np.int32), desc=f(o, o + NB * A).reshape(A, ref.RINGS, ref.SECTORS),
                ring_key=f(o + NB * A, o + (NB + ref.RINGS) * A).reshape(A, ref.RINGS),
                sector_key=f(o + (NB + ref.RINGS) * A, o + (NB + ref.RINGS + ref.SECTORS) * A).reshape(A, ref.SECTORS))


def parse_match(tok):
    Q, P = int(tok[2]), int(tok[3])
    v = tok[4:]
    i = lambda a, b: np.array([int(x) for x in v[a:b]], np.int32)
    f = lambda a, b: np.array([float(x) for x in v[a:b]])
    return dict(best_cand=i(0, Q), best_dist=f(Q, 2 * Q), best_shift=i(2 * Q, 3 * Q), yaw=f(3 * Q, 4 * Q), dist_all=f(4 * Q, 4 * Q + P),
                shift_all=i(4 * Q + P, 4 * Q + 2 * P))


def _compile(tmp_path_factory, flags, name):
    exe = str(tmp_path_factory.mktemp("scan_context") / name)
    # -ffp-contract=off: the header's pragma is clang's; GCC gets the same rule from the command line (scan_context.h, "Bits")
    out = subprocess.run(["g++", "-std=c++17", "-Wall", "-ffp-contract=off", "-I", INC, SRC, "-o", exe] + flags, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-4000:]
    return exe


@pytest.fixture(scope="module")
def core(tmp_path_factory):
    return _compile(tmp_path_factory, ["-O2"], "test_scan_context")


def comparable(res, rev=None):
    """The condition on the input: every decision of the restatement's result `res` (of describe or of match) is far above rounding;
    with `rev` (the result under the reversed summation order) also that both orders decide alike."""
    if "margin" in res:
        assert res["margin"] > 1e-9, res["margin"]
    else:
        for gap in ("align_gap", "shift_gap", "cand_gap", "tree_gap", "thres_gap"):
            assert res[gap] > 1e-9, (gap, res[gap])
        if rev is not None:
            for k in ("best_cand", "best_shift", "shift_all", "taken"):
                assert (res[k] == rev[k]).all(), k
    return res


def check_match(got, res, rev, who):
    """got: parse_match's dict of one set (or the device's).  Decisions equal, quantities within the bound; returns the ratios."""
    Q, C = res["dist_all"].shape
    assert (got["best_cand"] == res["best_cand"]).all() and (got["best_shift"] == res["best_shift"]).all(), (who, got["best_cand"], res["best_cand"])
    assert (np.asarray(got["shift_all"]).reshape(Q, C) == res["shift_all"]).all(), who
    return {k: ref.check(np.asarray(got[k]).reshape(res[k].shape), res[k], rev[k], f"{who} {k}") for k in ("dist_all", "best_dist", "yaw")}


# three members under non-trivial transforms: the scan of A seen through a small motion each
MOTIONS = [np.hstack([ref.rotz(3.0), [[0.4], [-0.2], [0.05]]]), np.hstack([ref.rotz(-7.5), [[-0.7], [0.3], [-0.02]]]),
           np.hstack([ref.rotz(1.0) @ np.array([[1, 0, 0], [0, np.cos(0.02), -np.sin(0.02)], [0, np.sin(0.02), np.cos(0.02)]]), [[0.1], [0.9], [0.0]]])]


def aggregate_cases():
    names = list(ref.VIEWS)
    scans = [ref.scan(n) for n in names]
    return scans, [[(0, MOTIONS[0]), (1, MOTIONS[1]), (2, MOTIONS[2])], [(0, None)] * 1, [(3, MOTIONS[1]), (0, MOTIONS[2]), (4, MOTIONS[0])]]


# ---- describe ---------------------------------------------------------------------------------------------------------------------------
def test_describe_against_restatement(core, tmp_path):
    """Identity members (the five views, one aggregate each) and aggregates of three members under non-trivial member_T: descriptors and
    n_binned equal the restatement's bit for bit; the keys within the bound.  Measured (g++ -O2): smallest bin margin 5.3e-7 (identity)
    and 8.7e-6 (three members); difference / bound: ring_key 0.125 at most, sector_key 0 (no difference: the restatement's column mean
    adds in ring order too); the restatement's own difference under the reversed order is 1.3e-15 at most."""
    names = list(ref.VIEWS)
    res = comparable(ref.descriptors())
    scans, aggs = aggregate_cases()
    agg_T = [[(k, ref.EYE if T is None else T) for k, T in a] for a in aggs]
    res3 = comparable(ref.describe(scans, agg_T))
    rows = run_program(core, [describe_command(scans, [[(k, None)] for k in range(len(names))]), describe_command(scans, agg_T)], tmp_path)
    print(f"bin margins: identity {res['margin']:.3e}, three members {res3['margin']:.3e}")
    for want, tok, who in ((res, rows[0], "identity"), (res3, rows[1], "three members")):
        A = len(want["desc"])
        got = parse_describe(tok, A)
        assert (got["n_binned"] == want["n_binned"]).all() and want["n_binned"].min() > 1000, who
        assert got["desc"].tobytes() == want["desc"].tobytes(), (who, np.abs(got["desc"] - want["desc"]).max())
        for a in range(A):
            rk, sk = ref.keys(want["desc"][a][::-1, ::-1])            # the restatement's own keys, summed in the other order
            ref.check(got["ring_key"][a], want["ring_key"][a], rk[::-1], f"{who} ring_key {a}")
            ref.check(got["sector_key"][a], want["sector_key"][a], sk[::-1], f"{who} sector_key {a}")


def test_sector_and_ring_rule_on_placed_points(core, tmp_path):
    """Points placed by construction: the four axes, 45 degrees and its mirror images, 1e-3 degrees either side of several 6-degree
    boundaries, r == max_radius and just beyond it, the origin."""
    R = 10.0
    pts, want = [], []

    def put(x, y, ring, sector):
        pts.append((x, y)); want.append(-1 if ring < 0 else ring * 60 + sector)

    put(3.0, 0.0, 5, 0); put(0.0, 3.0, 5, 14); put(-3.0, 0.0, 5, 29); put(0.0, -3.0, 5, 44)      # 0, 90, 180, 270: (84, 90] is sector 14
    put(2.0, 2.0, 5, 7); put(-2.0, 2.0, 5, 22); put(-2.0, -2.0, 5, 37); put(2.0, -2.0, 5, 52)    # 45 in (42, 48], 135, 225, 315
    for k in (1, 7, 8, 14, 15, 16, 29, 30, 31, 44, 45, 46, 52, 59):
        for eps, sector in ((-1e-3, k - 1), (1e-3, k)):
            a = np.radians(6.0 * k + eps)
            put(4.2 * np.cos(a), 4.2 * np.sin(a), 8, sector)
    a = np.radians(1e-3)
    put(4.2 * np.cos(a), -4.2 * np.sin(a), 8, 59); put(4.2 * np.cos(a), 4.2 * np.sin(a), 8, 0)   # either side of azimuth 0
    put(R, 0.0, 19, 0); put(0.0, -R, 19, 44); put(6.0, 8.0, 19, 8)                               # r == max_radius (6-8-10: exact) is kept
    put(np.nextafter(R, 20.0), 0.0, -1, 0); put(6.0, np.nextafter(8.0, 9.0), -1, 0)              # just beyond it
    put(0.0, 0.0, 0, 0)                                                                          # the origin
    put(0.5, 0.0, 0, 0); put(np.nextafter(0.5, 1.0), 0.0, 1, 0); put(1e-300, 1e-300, 0, 7)       # ring boundaries: (0, 0.5] is ring 0
    got = [int(t) for t in run_program(core, [bin_command(pts, R)], tmp_path)[0][2:]]
    assert got == want, [(p, g, w) for p, g, w in zip(pts, got, want) if g != w]
    # and the restatement agrees wherever arctan2 can be trusted (every point but those exactly on a boundary)
    ring, sector, margin = ref.bins(np.array([(x, y, 0.0) for x, y in pts]), R)
    sure = margin > 1e-9
    assert sure.sum() >= 30 and (np.where(ring < 0, -1, ring * 60 + sector)[sure] == np.array(want)[sure]).all()


def test_empty_aggregates_and_points_beyond_the_radius(core, tmp_path):
    """No member, a member whose scan is empty, every point beyond the radius: all zeros, n_binned 0; a scan used by two aggregates."""
    far = np.array(ref.scan("A")) * 100.0
    scans = [ref.scan("A"), np.zeros((0, 3)), far]
    got = parse_describe(run_program(core, [describe_command(scans, [[], [(1, None)], [(2, None)], [(0, None)], [(0, None), (1, None)]])], tmp_path)[0], 5)
    for a in range(3):
        assert got["n_binned"][a] == 0 and not got["desc"][a].any() and not got["ring_key"][a].any() and not got["sector_key"][a].any()
    assert got["n_binned"][3] == got["n_binned"][4] > 0 and got["desc"][3].tobytes() == got["desc"][4].tobytes()
    assert got["desc"][3].tobytes() == ref.descriptors()["desc"][0].tobytes()


def test_negative_heights_and_empty_bins(core, tmp_path):
    """A bin's value is the maximum even when it is negative; a bin without a point is 0."""
    pts = np.array([[1.0, 0.5, -3.0], [1.1, 0.5, -2.5], [5.0, 5.0, 1.0]])
    got = parse_describe(run_program(core, [describe_command([pts], [[(0, None)]], lidar_height=2.0, max_radius=20.0)], tmp_path)[0], 1)
    want = ref.describe([pts], [[(0, None)]], 2.0, 20.0)
    assert got["desc"].tobytes() == want["desc"].tobytes() and got["desc"][0, 1, 4] == -0.5 and got["desc"][0, 7, 7] == 3.0
    assert np.count_nonzero(got["desc"]) == 2 and got["n_binned"][0] == 3


# ---- match ------------------------------------------------------------------------------------------------------------------------------
# name -> (queries, candidates, parameters other than the shipped ones).  The first four: A against (A revisited, A from afar, B, C),
# which finds the revisit.  The last three hold no revisit: every best distance is finite and NOT below dist_thres, so best_cand is -1
# while best_dist and best_shift are still reported.
REST = ("A_revisit", "A_far", "B", "C")
MATCH_CASES = {"shipped": (("A",), REST, dict()), "all": (("A",), REST, dict(n_tree_candidates=0)), "K2": (("A",), REST, dict(n_tree_candidates=2)),
               "full_window": (("A",), REST, dict(search_ratio=1.0, n_tree_candidates=0)),
               "none_BC": (("B", "C"), ("A", "A_revisit", "A_far"), dict()),
               "none_BC_full_window": (("B", "C"), ("A", "A_revisit", "A_far"), dict(search_ratio=1.0, n_tree_candidates=0)),
               "none_A_K2": (("A",), ("A_far", "B", "C"), dict(n_tree_candidates=2))}


def match_case(name):
    """(query descriptors, candidate descriptors, parameters, the restatement's result, its result under the reversed order) of a case,
    after asserting that the case can be compared; a case without a revisit must say -1 for finite distances."""
    query, cands, kw = MATCH_CASES[name]
    res, rev = ref.matched(query, cands, **kw), ref.matched(query, cands, rev=True, **kw)
    comparable(res, rev)
    if name.startswith("none"):
        thres = ref.DEFAULTS["dist_thres"]
        assert (res["best_cand"] == -1).all() and np.isfinite(res["best_dist"]).all() and (res["best_dist"] > thres).all() and res["thres_gap"] > 1e-9
    D, idx = ref.descriptors()["desc"], {n: k for k, n in enumerate(ref.VIEWS)}
    return D[[idx[n] for n in query]], D[[idx[n] for n in cands]], dict(ref.DEFAULTS, **kw), res, rev


@pytest.mark.parametrize("name", list(MATCH_CASES))
def test_match_against_restatement(name, core, tmp_path):
    """A against (A revisited, A from afar, B, C); then the cases without a revisit, whose -1 decisions, best_dist and best_shift are the
    restatement's (B and C against the three views of A: best distances 0.61 and 0.96, 0.49 and 0.96 with the full window; A against (A from afar,
    B, C) with K = 2: 0.74; threshold gap at least 0.19; difference / bound 0.125 at most, yaw 0.68).
    Measured (g++ -O2): distances 0.087 (shift 15), 0.815, 0.736, 0.961 (full
    window: 0.087, 0.718, 0.679, 0.960); alignment gap 5.8e-3, shift gap 1.5e-4 (5.6e-5 with the full window), candidate gap 0.65 (0.59),
    ring-key gap 0.27 (K = 2), threshold gap 0.21; difference / bound: dist_all 0.125 at most, best_dist 0, yaw 0.64 (its bound is the
    2^-52 floor: the restatement's own difference is 0 there and 1.1e-16 in the distances)."""
    q, c, kw, res, rev = match_case(name)
    got = parse_match(run_program(core, [match_command([(q, c)], **kw)], tmp_path)[0])
    print(name, "dist", res["dist_all"], "shift", res["shift_all"], {g: res[g] for g in ("align_gap", "shift_gap", "cand_gap", "tree_gap", "thres_gap")})
    check_match(got, res, rev, f"header {name}")
    if name.startswith("none"):
        assert (got["best_cand"] == -1).all() and (got["best_shift"] == res["best_shift"]).all() and np.isfinite(got["best_dist"]).all()
    else:
        assert got["best_cand"][0] == 0 and got["best_shift"][0] in (15, 16)     # the revisit: 93 degrees are 15.5 sectors


def test_refinement_window(core, tmp_path):
    """R = 3 (ratio 0.1) finds the revisit; search_ratio 1 equals brute force over all 60 shifts; R = 0 compares shift0 alone."""
    D = ref.descriptors()["desc"]
    q, c = D[[0]], D[[1]]
    ratios = (0.1, 1.0, 0.0, 5.0)
    assert [ref.search_radius(r) for r in ratios] == [3, 30, 0, 30]
    rows = run_program(core, [match_command([(q, c)], 0, ratio, 0.3) for ratio in ratios], tmp_path)
    got = [parse_match(t) for t in rows]
    for ratio, g in zip(ratios, got):
        res, rev = ref.match(q, c, 0, ratio, 0.3), ref.match(q, c, 0, ratio, 0.3, rev=True)
        comparable(res, rev)
        check_match(g, res, rev, f"header ratio {ratio}")
    brute = ref.compare(q[0], c[0], 30)
    assert len(brute[4]) == 60 and min(brute[4], key=brute[4].get) == brute[1] == got[1]["best_shift"][0] == got[0]["best_shift"][0] and brute[1] in (15, 16)
    assert got[1]["dist_all"].tobytes() == got[3]["dist_all"].tobytes() == got[0]["dist_all"].tobytes()


def test_preselection(core, tmp_path):
    """K = 2 leaves out the right candidates (those farthest in ring-key distance) and gives them +infinity; K = 0, K = n and K > n
    agree; several queries and two sets in one command."""
    D = ref.descriptors()["desc"]
    cands = D[[1, 2, 3, 4]]
    res = comparable(ref.matched(n_tree_candidates=2))
    assert res["taken"].sum() == 2 and res["taken"][0, 0]
    rows = run_program(core, [match_command([(D[[0]], cands)], K) for K in (2, 0, 4, 64, -3)], tmp_path)
    got = [parse_match(t) for t in rows]
    assert (np.isinf(got[0]["dist_all"]) == ~res["taken"][0]).all() and (got[0]["shift_all"][~res["taken"][0]] == 0).all()
    for g in got[2:]:
        for k in got[1]:
            assert g[k].tobytes() == got[1][k].tobytes(), k
    assert np.isfinite(got[1]["dist_all"]).all()
    # two sets, three queries: per query the bits of its lone command
    sets = [(D[[0, 3]], cands), (D[[4]], D[[2, 1]])]
    both = parse_match(run_program(core, [match_command(sets, 2)], tmp_path)[0])
    lone = [parse_match(t) for t in run_program(core, [match_command([(D[[0]], cands)], 2), match_command([(D[[3]], cands)], 2),
                                                       match_command([(D[[4]], D[[2, 1]])], 2)], tmp_path)]
    assert both["dist_all"].tobytes() == np.concatenate([g["dist_all"] for g in lone]).tobytes()
    for k in ("best_cand", "best_dist", "best_shift", "yaw"):
        assert both[k].tobytes() == np.concatenate([g[k] for g in lone]).tobytes(), k
    assert both["best_cand"][1] == 2 and abs(both["best_dist"][1]) < 1e-15 and both["best_shift"][1] == 0   # B among the candidates: itself


def test_all_zero_descriptors_and_empty_sets(core, tmp_path):
    """An all-zero query or candidate gives +infinity and -1; a set without candidates gives -1, +infinity, shift 0; a set without
    queries and a command without sets give nothing."""
    D = ref.descriptors()["desc"]
    zero = np.zeros((1, ref.RINGS, ref.SECTORS))
    rows = run_program(core, [match_command([(zero, D[[0, 2]])], 0), match_command([(D[[1]], zero)], 0), match_command([(D[[1]], D[:0])], 10),
                              match_command([(D[:0], D[[0]])], 10), match_command([], 10),
                              match_command([(D[[0]], np.concatenate([zero, D[[1]]]))], 0)], tmp_path)
    got = [parse_match(t) for t in rows]
    for g in got[:2]:
        assert g["best_cand"][0] == -1 and np.isinf(g["best_dist"][0]) and np.isinf(g["dist_all"]).all()
    assert got[2]["best_cand"][0] == -1 and np.isinf(got[2]["best_dist"][0]) and got[2]["best_shift"][0] == 0 and got[2]["yaw"][0] == 0.0
    assert len(got[3]["best_cand"]) == 0 and len(got[4]["best_cand"]) == 0
    assert got[5]["best_cand"][0] == 1 and np.isinf(got[5]["dist_all"][0]) and got[5]["best_shift"][0] in (15, 16)


def extreme_sets():
    """Finite descriptors near the ends of the FP64 range, where a ring-key distance, an alignment norm or a cosine can be NaN (a sum
    that overflows, then inf - inf; a product of norms that underflows, then 0 / 0): A revisited scaled to 1e306, 1e-162 and 1e-170
    among (A from afar, B, C), A as the query and, in a second set, the 1e306 descriptor as the query."""
    D = ref.descriptors()["desc"]
    huge, tiny, gone = D[1] * (1e306 / D[1].max()), D[1] * 1e-162, D[1] * 1e-170
    cands = np.stack([huge, D[2], tiny, D[3], gone, D[4]])
    assert np.isfinite(cands).all()
    return [(D[[0]], cands), (huge[None], cands)]


def test_nan_counts_as_infinity(core, tmp_path):
    """Every comparison of the search has a total order: with K = 2 .. 5 exactly K candidates are compared whatever overflows, no
    distance is NaN, and the all-candidates call still finds the plain ones."""
    sets = extreme_sets()
    for K in (0, 2, 3, 5):
        got = parse_match(run_program(core, [match_command(sets, K, 0.1, 0.3)], tmp_path)[0])
        assert not np.isnan(got["dist_all"]).any() and not np.isnan(got["best_dist"]).any()
        if K:
            assert (np.isfinite(got["dist_all"]).reshape(2, 6).sum(axis=1) <= K).all() and ((got["shift_all"].reshape(2, 6) != 0).sum(axis=1) <= K).all()
    assert np.isfinite(got["dist_all"][[1, 3, 5]]).all()


def test_header_under_sanitizers(tmp_path_factory, tmp_path):
    """The header as a stand-alone host program under AddressSanitizer and UndefinedBehaviorSanitizer, arrays of exact size: the smallest
    cases of every command run clean."""
    exe = _compile(tmp_path_factory, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "test_scan_context_san")
    D = ref.descriptors()["desc"]
    A = np.array(ref.scan("A"))
    zero = np.zeros((1, ref.RINGS, ref.SECTORS))
    cmds = [describe_command([A[:257], A[:0], A[:1] * 1000.0], [[(0, MOTIONS[0]), (1, MOTIONS[1])], [], [(2, MOTIONS[2])], [(0, MOTIONS[2])]]),
            describe_command([A[:300]], [[(0, None)]]), describe_command([], []), describe_command([A[:3]], []),
            match_command([(D[[0]], D[[1, 2, 3, 4]])], 2), match_command([(D[[1, 3]], D[[0, 2]]), (D[[4]], D[:0]), (D[:0], D[[0]])], 0, 1.0),
            match_command([], 10), match_command([(zero, zero)], 1, 0.0), match_command(extreme_sets(), 3),
            bin_command([(0.0, 0.0), (1.0, 0.0), (0.0, -1.0), (-7.0, 7.0), (1e308, 1e308), (11.0, 0.0)], 10.0)]
    run_program(exe, cmds, tmp_path)


def test_declared_and_bound():
    """The C-ABI declares the entry points and the Python side binds them with the contract's constants."""
    from beam_slam_amd import capi, gpu
    text = open(os.path.join(ROOT, "include", "bsgpu.h")).read()
    assert "int bsgpu_scan_context_describe(int device, int32_t n_scans" in text and "int bsgpu_scan_context_match(int device, int32_t n_sets" in text
    for s in ("scan_context_describe", "scan_context_match", "scan_context_error"):
        assert s in capi.SYMBOLS
    assert "#define BSGPU_SC_RINGS 20" in text and "#define BSGPU_SC_SECTORS 60" in text and "#define BSGPU_SC_MAX_CANDIDATES 65536" in text
    assert "#define BSGPU_SC_MAX_TREE_CANDIDATES 64" in text and "#define BSGPU_SC_MAX_SCAN_POINTS (65535 * 4096)" in text
    assert capi.SC_MAX_SCAN_POINTS == 65535 * 4096
    assert (capi.SC_RINGS, capi.SC_SECTORS, capi.SC_MAX_CANDIDATES, capi.SC_MAX_TREE_CANDIDATES) == (ref.RINGS, ref.SECTORS, 65536, 64)
    assert len(capi.SCAN_CONTEXT_DESCRIBE_ARGTYPES) == 14 and len(capi.SCAN_CONTEXT_MATCH_ARGTYPES) == 15
    assert callable(gpu.scan_context_describe) and callable(gpu.scan_context_match)
    assert {k: capi.SC_DEFAULTS[k] for k in ref.DEFAULTS} == ref.DEFAULTS
    for word in ("-1000", "NUM_EXCLUDE_RECENT", "RECALLED", "divides by zero"):
        assert word in text
