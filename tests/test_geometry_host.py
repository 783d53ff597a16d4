"""CPU: the host side of the posterior geometry report -- diagnostics.geometry_from_sums and coupling_from_sums on sums
built in numpy, the flag, analyze --geometry on a hand-written results directory, the header and the binding."""
import json
import os
import re

import numpy as np
import pytest

import geometry_ref as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sums_from(mean, cov, n, shift=None):
    """The [D + 2, D] sums of n rows whose sample mean and sample covariance are exactly (mean, cov), about `shift`."""
    mean, cov = np.asarray(mean, np.float64), np.asarray(cov, np.float64)
    D = mean.size
    m = mean - (np.zeros(D) if shift is None else np.asarray(shift, np.float64))
    s = np.zeros((D + 2, D))
    s[:D] = (n - 1) * cov + n * np.outer(m, m)
    s[D] = n * m
    s[D + 1, 0] = n
    return s


def _ar1(D, rho):
    i = np.arange(D)
    return rho ** np.abs(i[:, None] - i[None, :])


def test_ar1_correlation_has_its_closed_form_eigenvalues():
    """AR(1), rho = 0.9, D = 16: R's inverse is tridiagonal, and its eigenvalues are (1 - rho^2) / (1 - 2 rho cos t + rho^2)
    at the D roots t of  sin((D + 1) t) - 2 rho sin(D t) + rho^2 sin((D - 1) t) = 0  in (0, pi) (Grenander & Szego); here
    they are found by bisection between the sign changes of that function."""
    from autoreparam_amd import diagnostics
    D, rho, n = 16, 0.9, 1000
    sd = np.linspace(0.5, 20.0, D)
    mean = np.linspace(-3.0, 3.0, D)
    shift = mean + 0.1
    g = diagnostics.geometry_from_sums(_sums_from(mean, _ar1(D, rho) * np.outer(sd, sd), n, shift), shift=shift)
    f = lambda t: np.sin((D + 1) * t) - 2 * rho * np.sin(D * t) + rho * rho * np.sin((D - 1) * t)
    grid = np.linspace(1e-6, np.pi - 1e-6, 20001)
    roots = []
    for a, b in zip(grid[:-1], grid[1:]):
        if f(a) * f(b) < 0:
            for _ in range(80):
                c = 0.5 * (a + b)
                a, b = (c, b) if f(a) * f(c) > 0 else (a, c)
            roots.append(0.5 * (a + b))
    assert len(roots) == D
    lam = np.sort((1 - rho * rho) / (1 - 2 * rho * np.cos(np.array(roots)) + rho * rho))
    assert np.allclose(g.eigenvalues, lam, rtol=1e-9, atol=0)
    assert g.condition_number == pytest.approx(lam[-1] / lam[0], rel=1e-9)
    assert g.rows == n and len(g.left_out) == 0 and np.array_equal(g.kept, np.arange(D))
    assert np.allclose(g.mean, mean, atol=1e-12) and np.allclose(g.sd, sd, rtol=1e-12)
    assert np.allclose(g.correlation, _ar1(D, rho), atol=1e-12)
    assert g.max_abs_correlation == pytest.approx(rho, abs=1e-12) and g.max_correlation_pair[1] == g.max_correlation_pair[0] + 1
    # the soft direction of a positively correlated family has one sign; both are unit eigenvectors of R
    R = _ar1(D, rho)
    for v, l in ((g.softest_direction, lam[-1]), (g.stiffest_direction, lam[0])):
        assert abs(np.linalg.norm(v) - 1) < 1e-12 and np.allclose(R @ v, l * v, atol=1e-9)
    assert (g.softest_direction > 0).all() or (g.softest_direction < 0).all()
    assert g.step_scaled_eigenvalues is None and np.isnan(g.step_scaled_condition_number)


def test_constant_column_is_left_out_and_directions_are_expanded():
    from autoreparam_amd import diagnostics
    D, n = 5, 50
    cov = np.diag([4.0, 1.0, 0.0, 9.0, 1.0])
    cov[0, 1] = cov[1, 0] = 1.0                                 # correlation 0.5 between elements 0 and 1
    g = diagnostics.geometry_from_sums(_sums_from(np.arange(D, dtype=float), cov, n))
    assert list(g.left_out) == [2] and list(g.kept) == [0, 1, 3, 4]
    assert g.correlation.shape == (4, 4) and g.eigenvalues.shape == (4,) and np.isnan(g.sd[2])
    assert g.condition_number == pytest.approx(1.5 / 0.5, rel=1e-12)
    assert g.max_correlation_pair == (0, 1) and g.max_abs_correlation == pytest.approx(0.5)
    assert g.stiffest_direction.shape == (D,) and g.stiffest_direction[2] == 0 and g.softest_direction[2] == 0
    assert np.allclose(np.abs(g.stiffest_direction), [np.sqrt(0.5), np.sqrt(0.5), 0, 0, 0], atol=1e-12)


def test_eps0_gives_the_step_scaled_condition_number():
    """Independent elements with sd (1, 10, 100): R = I, condition number 1 -- but with equal steps the integrator works in
    a shape of condition number 10^4; steps proportional to the sd bring it back to 1."""
    from autoreparam_amd import diagnostics
    sd = np.array([1.0, 10.0, 100.0])
    s = _sums_from(np.zeros(3), np.diag(sd ** 2), 200)
    equal = diagnostics.geometry_from_sums(s, eps0=np.full(3, 0.1))
    fitted = diagnostics.geometry_from_sums(s, eps0=0.2 * sd)
    assert equal.condition_number == pytest.approx(1.0) and fitted.condition_number == pytest.approx(1.0)
    assert equal.step_scaled_condition_number == pytest.approx(1e4, rel=1e-12)
    assert np.allclose(equal.step_scaled_eigenvalues, sd ** 2 / 0.01, rtol=1e-12)
    assert fitted.step_scaled_condition_number == pytest.approx(1.0, rel=1e-12)
    assert np.allclose(fitted.step_scaled_eigenvalues, 25.0, rtol=1e-12)


def test_one_row_and_no_row_give_nan_not_an_exception():
    from autoreparam_amd import diagnostics
    D = 4
    for n in (0, 1):
        s = np.zeros((D + 2, D))
        s[D + 1, 0] = n
        if n:
            x = np.array([1.0, -2.0, 3.0, 0.5])
            s[:D], s[D] = np.outer(x, x), x
        g = diagnostics.geometry_from_sums(s, eps0=np.ones(D))
        assert g.rows == n and len(g.left_out) == D and g.kept.size == 0 and g.eigenvalues.size == 0
        assert np.isnan(g.condition_number) and np.isnan(g.step_scaled_condition_number) and np.isnan(g.max_abs_correlation)
        assert g.max_correlation_pair == (-1, -1) and np.isnan(g.sd).all() and not g.stiffest_direction.any()
    with pytest.raises(ValueError):
        diagnostics.geometry_from_sums(np.zeros((4, 4)))


def test_sums_from_rows_agree_with_the_reference_and_add():
    """geometry_from_sums on geometry_ref.gram_ref of random correlated rows equals geometry_ref.geometry_ref on the rows;
    the sums of two halves add; coupling_from_sums on the sums of [u, v] equals geometry_ref.coupling_ref."""
    from autoreparam_amd import diagnostics
    rs = np.random.RandomState(1)
    n, D = 4000, 6
    x = (rs.randn(n, D) @ rs.randn(D, D) + 5.0).astype(np.float32)
    shift = x[:10].mean(axis=0)
    eps0 = np.linspace(0.1, 0.6, D)
    whole = gr.gram_ref(x, shift)
    assert np.allclose(gr.gram_ref(x[:1500], shift) + gr.gram_ref(x[1500:], shift), whole, rtol=1e-12)
    g, ref = diagnostics.geometry_from_sums(whole, eps0=eps0, shift=shift), gr.geometry_ref(x, eps0)
    assert np.allclose(g.mean, ref["mean"], atol=1e-9) and np.allclose(g.sd, ref["sd"], rtol=1e-9)
    assert np.allclose(g.correlation, ref["correlation"], atol=1e-9) and np.allclose(g.eigenvalues, ref["eigenvalues"], rtol=1e-7)
    assert np.allclose(g.step_scaled_eigenvalues, ref["step_scaled_eigenvalues"], rtol=1e-7)
    assert g.max_correlation_pair == ref["pair"]
    u = (x.astype(np.float64) - ref["mean"]) / ref["sd"]
    both = np.concatenate([u, 0.5 * np.log(u * u + diagnostics.COUPLING_FLOOR)], axis=1)
    a = np.zeros((2 * D + 2, 2 * D))
    a[:2 * D], a[2 * D], a[2 * D + 1, 0] = both.T @ both, both.sum(axis=0), n
    K = diagnostics.coupling_from_sums(a)
    assert K.shape == (D, D) and not np.diag(K).any() and np.allclose(K, gr.coupling_ref(x), atol=1e-9)


def test_flag_defaults_and_parsing():
    from autoreparam_amd import flags as flags_mod
    f = flags_mod.FlagValues()
    assert f.geometry_diagnostics is False
    f.parse(["--geometry_diagnostics"])
    assert f.geometry_diagnostics is True
    f.parse(["--nogeometry_diagnostics"])
    assert f.geometry_diagnostics is False
    f.parse(["--geometry_diagnostics=true"])
    assert f.geometry_diagnostics is True
    text = [h for name, _, _, h in flags_mod._DEFS if name == "geometry_diagnostics"][0]
    assert "not a local metric" in text and "--convergence_diagnostics" in text


def test_chunks_and_element_names():
    from autoreparam_amd import main as cli
    import helpers
    assert cli.geometry_chunk_steps(1000, 65536, 71) == cli.GEOMETRY_CHUNK_BYTES // (12 * 65536 * 71) >= 1
    assert cli.geometry_chunk_steps(10, 4, 9) == 10 and cli.geometry_chunk_steps(1000, 1 << 22, 512) == 1
    sp = helpers.spec("8schools")
    names = cli.element_names(sp)
    assert len(names) == sp.D == len(set(names))
    vector = [n for n, s in zip(sp.part_names, sp.part_shapes) if len(s)][0]
    assert vector + "[0]" in names
    for n, s in zip(sp.part_names, sp.part_shapes):
        if not len(s):
            assert n in names


def test_analyze_geometry_on_a_hand_written_directory(tmp_path, capsys):
    from autoreparam_amd import analyze
    d = tmp_path / "radon_MN"
    d.mkdir()
    one = {"geometry_rows": [5, 1000], "geometry_rows_left_out": [0, 2], "geometry_chains": [5, 10],
           "geometry_elements_left_out": [0, 0], "geometry_condition_number": [9.0, 123.4],
           "geometry_condition_number_step_scaled": [9.0, 55.5], "geometry_condition_number_centred": [9.0, 4321.0],
           "geometry_max_abs_correlation": [0.1, 0.93], "geometry_max_correlation_pair": [None, ["a[0]", "mu"]],
           "geometry_max_scale_coupling": [0.0, 0.71], "geometry_max_scale_coupling_pair": [None, ["log_tau", "a[3]"]],
           "geometry_time_sec": [0.1, 0.25], "ess_min": [1.0, 1.0]}
    two = dict(one)
    keys = ("geometry_elements_left_out", "geometry_condition_number", "geometry_condition_number_step_scaled",
            "geometry_max_abs_correlation", "geometry_max_correlation_pair", "geometry_max_scale_coupling",
            "geometry_max_scale_coupling_pair")
    k0 = {k: one[k][-1] for k in keys}
    two["geometry_by_kernel"] = [None, [k0, dict(k0, geometry_condition_number=None, geometry_max_correlation_pair=None)]]
    json.dump(one, open(str(d / "NCP_tied.json"), "w"))
    json.dump(two, open(str(d / "i_tied.json"), "w"))
    json.dump({"ess_min": [1.0]}, open(str(d / "CP_tied.json"), "w"))
    np.savez(str(d / "NCP_tied_geometry.npz"), elements=np.asarray(["mu", "log_tau", "a[0]", "a[1]"]),
             **{"stiffest_direction/mu": np.float64(0.1), "stiffest_direction/log_tau": np.float64(-0.9),
                "stiffest_direction/a": np.asarray([0.3, 0.3])})
    lines = analyze.report_geometry(analyze.load(str(tmp_path), "radon_MN"), str(tmp_path), "radon_MN")
    head = [l for l in lines if not l.startswith(" ")]
    assert len(head) == 3 and not any(l.startswith("CP") for l in lines)
    ncp = [l for l in head if l.startswith("NCP_tied")][0]
    for piece in ("123.4", "55.5", "4321", "0.93", "a[0] ~ mu", "0.71", "log_tau -> a[3]", "1000 draws of 10 chains", "2 left out"):
        assert piece in ncp, piece
    assert any(l.startswith("i_tied kernel 1") and "condition number n/a" in l and "(n/a)" in l for l in head)
    stiff = [l for l in lines if "stiffest direction" in l]
    assert len(stiff) == 1 and stiff[0].index("log_tau -0.900") < stiff[0].index("a[0] +0.300")
    analyze.main(["--results_dir=" + str(tmp_path), "--model=radon_MN", "--geometry"])
    assert "NCP_tied: condition number 123.4" in capsys.readouterr().out


def test_header_declares_and_binding_lists_the_symbols():
    from autoreparam_amd import _lib
    src = open(os.path.join(ROOT, "include", "autoreparam.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("arp_gram_workspace_bytes", "arp_gram_sums"):
        assert re.search(r"\b%s\s*\(" % name, code) and name in _lib.SYMBOLS
    assert re.search(r"#define\s+ARP_ABI_VERSION\s+2\b", src)


def test_header_comment_carries_the_bound_and_the_rules():
    from autoreparam_amd import diagnostics
    src = open(os.path.join(ROOT, "include", "autoreparam.h")).read()
    doc = [c for c in re.findall(r"/\*.*?\*/", src, flags=re.S) if "arp_gram_workspace_bytes" in c]
    assert len(doc) == 1
    doc = " ".join(doc[0].replace("*", " ").split())
    assert "|G_dev - G_f64|[i][j] <= (kGramWindow + 1) 2^-24 sum_r |u_ri u_rj|" in doc
    assert "by select, never by a multiplication" in doc and "0 inf is NaN" in doc
    assert "no atomics" in doc and "bitwise equal" in doc and "bitwise the sums of its contiguous copy" in doc
    kernel = open(os.path.join(ROOT, "autoreparam_amd", "csrc", "gram.hip")).read()
    m = re.search(r"constexpr int kGramWindow = (\d+);", kernel)
    assert m and int(m.group(1)) == diagnostics.GRAM_WINDOW == gr.W <= 256
    for phrase in ("Zeroed operands", "Reads past the end", "Rows left out"):
        assert phrase in kernel
