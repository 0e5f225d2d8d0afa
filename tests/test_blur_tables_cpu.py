"""blur_tables() (csrc/blur.hip) on the host: the stand-alone checker tests/host/blur_tables_check.cpp is built into
tmp_path -- host code only, under the address and undefined-behaviour sanitizers -- and run as a child process over the
named degenerate families and a seeded fuzz set (tests/blur_families.py).  Nothing is loaded into this process."""
import glob
import json
import os
import shutil
import subprocess
import time

import numpy as np
import pytest
import yaml

import blur_families as bf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    """-> run(records) -> one dict per record; records: list of (kernel, mode)"""
    tmp = tmp_path_factory.mktemp("blur_tables")
    exe = str(tmp / "blur_tables_check")
    t0 = time.time()
    # the sanitizers are for the host code alone: each such flag is scoped to the host with -Xarch_host
    host_san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"]
    subprocess.run([HIPCC, "-x", "hip", "--offload-host-only", *host_san, "-g", "-O1", "-std=c++17", "-ffp-contract=off", "-Wl,--unresolved-symbols=ignore-all",
                    "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "dps_ttc_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "blur_tables_check.cpp"), "-o", exe],
                   check=True, cwd=str(tmp))
    print(f"host checker built in {time.time() - t0:.1f} s")
    count = [0]

    def run(records):
        count[0] += 1
        path = str(tmp / f"records{count[0]}.bin")
        bf.write_records(path, records)
        t1 = time.time()
        p = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        os.remove(path)
        assert p.returncode == 0 and p.stderr == "", f"checker exit {p.returncode}:\n{p.stderr[-4000:]}"
        rows = [json.loads(line) for line in p.stdout.splitlines()]
        print(f"host checker: {len(rows)} records in {time.time() - t1:.1f} s")
        assert len(rows) == len(records)
        for row, (k, mode) in zip(rows, records):
            assert row["ks"] == k.shape[0] and row["mode"] == mode
        return rows

    return run


def _violations(rows, names):
    return [(names[r["i"]], r["viol"]) for r in rows if r["viol"]]


def test_named_families_tables_hold(checker):
    fam = bf.named_families()
    records = [(k, mode) for _, _, k, _ in fam for mode in (bf.AUTO, bf.FORCE_TAPS)]
    names = [f"{f}.{name}/{mode}" for f, name, _, _ in fam for mode in ("auto", "taps")]
    rows = checker(records)
    assert _violations(rows, names) == []
    # the rank-1 members are separable exactly in AUTO; nothing else is in either mode
    for n, (_, name, _, rank1) in enumerate(fam):
        assert rows[2 * n]["separable"] == rank1, name
        assert rows[2 * n + 1]["separable"] is False, name


def test_fuzz_tables_hold(checker):
    kernels = bf.fuzz_kernels()
    assert len(kernels) == len(bf.FUZZ_SIZES) * bf.FUZZ_PER_SIZE
    records = [(k, mode) for k in kernels for mode in (bf.AUTO, bf.FORCE_TAPS)]
    names = [f"fuzz{n}.ks{k.shape[0]}/{mode}" for n, k in enumerate(kernels) for mode in ("auto", "taps")]
    rows = checker(records)
    assert _violations(rows, names) == []
    # the set is what it claims to be: the separable branch, the all-zero kernel and every run class are in it
    assert sum(r["separable"] for r in rows) >= 50
    assert any(r["nrun"] == [0, 0, 0, 0] for r in rows)
    assert all(any(r["nrun"][c] > 0 for r in rows) for c in range(4))


ROUTE_FACTS = {"swc_fwd": (100, 132), "swc_adj": (100, 132), "nhb2": (False, True), "strip16": (False, True),
               "multipass": (False, True), "sym": (False, True), "empty0": (False, True), "empty1": (False, True),
               "empty2": (False, True), "empty3": (False, True)}


def route_coverage(rows):
    """-> {fact: {value: count}} over the checker's rows"""
    cov = {f: {v: 0 for v in vals} for f, vals in ROUTE_FACTS.items()}
    for r in rows:
        facts = dict(r, **{f"empty{c}": r["empty"][c] for c in range(4)})
        for f in ROUTE_FACTS:
            if facts[f] is not None:            # sym: separable handles only
                cov[f][facts[f]] += 1
    return cov


def test_named_families_reach_every_route(checker):
    """every value of every fact the launchers branch on -- the LDS stride class of the forward and of the one-launch
    adjoint, the 2- or 4-unit halo loader, 16- or 32-column strips, the multi-pass fallback, the symmetric separable
    adjoint, each run class empty or not -- occurs among the named families: the device tests run what this lists"""
    fam = bf.named_families()
    rows = checker([(k, mode) for _, _, k, _ in fam for mode in (bf.AUTO, bf.FORCE_TAPS)])
    cov = route_coverage(rows)
    print(json.dumps({f: {str(v): n for v, n in c.items()} for f, c in cov.items()}))
    missing = [(f, v) for f, c in cov.items() for v, n in c.items() if n == 0]
    assert missing == []


def _shipped_gaussians():
    out = set()
    for path in sorted(glob.glob(os.path.join(ROOT, "configs", "*.yaml"))):
        with open(path) as f:
            cfg = yaml.load(f, Loader=yaml.FullLoader)        # (the inpainting config holds a python/tuple)
        op = ((cfg or {}).get("measurement") or {}).get("operator") or {}
        if op.get("name") == "gaussian_blur":
            out.add((int(op["kernel_size"]), float(op["intensity"])))
    return sorted(out)


def test_shipped_gaussians_stay_separable(checker):
    from oracle.tables import gaussian_kernel2d
    pairs = _shipped_gaussians()
    assert (61, 3.0) in pairs
    rows = checker([(gaussian_kernel2d(ks, sigma).astype(np.float32), bf.AUTO) for ks, sigma in pairs])
    for (ks, sigma), r in zip(pairs, rows):
        assert r["viol"] == [] and r["separable"] is True and r["sym"] is True, (ks, sigma, r)


def test_rank1_bound_is_on_the_operator(checker):
    """the pedestal kernel passes an element-wise 1e-6 * peak test and is 4.6e-5 away in relative L1: no longer
    separable; the asymmetric rank-1 products other tests assert KIND_SEP for stay separable"""
    from oracle.tables import gaussian_kernel2d
    ped = bf.pedestal_kernel()
    g = gaussian_kernel2d(61, 3.0)
    # the premise, recomputed: within the old element-wise bound, far outside the new one
    pi, pj = np.unravel_index(np.argmax(np.abs(ped)), ped.shape)
    col = ped[:, pj].astype(np.float64)
    row = (ped[pi, :].astype(np.float64) / float(ped[pi, pj])).astype(np.float32).astype(np.float64)
    diff = np.abs(np.outer(col, row) - ped.astype(np.float64))
    assert diff.max() <= 1e-6 * float(np.abs(ped).max())
    assert 4e-5 < diff.sum() / np.abs(ped.astype(np.float64)).sum() < 5e-5
    named = bf.asymmetric_rank1_kernels()
    rows = checker([(ped, bf.AUTO), (g.astype(np.float32), bf.AUTO)] + [(k, bf.AUTO) for _, k in named])
    assert rows[0]["viol"] == [] and rows[0]["separable"] is False
    assert rows[1]["separable"] is True
    for (name, _), r in zip(named, rows[2:]):
        assert r["viol"] == [] and r["separable"] is True, name
