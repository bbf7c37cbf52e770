"""Which kernel a 4-bit GEMM shape runs, without a GPU: cgemm_4bit_plan reports the launch plan of
cgemm_4bit_inference_ws_* (gemm4bit.hip fewtoken_plan; without a device the CU count is the MI355X's 256).

tests/golden/fewtoken_plan_v1.json was recorded from a kernel trace of real launches (tools/fewtoken_plan_dump.py under
rocprofv3 --kernel-trace): per row the kernel with its template arguments after T, the workgroups, the threads per
workgroup and the reduce kernel that followed.  The plan must name exactly that with every knob at its default, and the
kernel each test knob forces on the shapes the GPU tests use it on."""
import ctypes as ct
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "fewtoken_plan_v1.json")
# FtKernel (csrc/gemm_common.hpp)
NONE, BAD_ARGS, GEMV_TOK, T64, T64R, FEWTOK, WK, SKINNY, TILE128, TILE256 = range(10)
FIELDS = ("kernel", "grid", "threads", "splits", "kchunk", "mt", "rg", "waves", "s4", "x8", "cfg", "lds", "reduce")


def _lib():
    import python_src_quants as bnb
    assert bnb.HIP_AVAILABLE, "libbitsandbytes_hip.so did not load"
    return bnb.lib


def _plan(N, rows, K, blocksize=64, blocksize2=256, nested=True):
    out = (ct.c_int * 16)()
    _lib().cgemm_4bit_plan(ct.c_int(N), ct.c_int(rows), ct.c_int(K), ct.c_int(blocksize),
                           ct.c_int(blocksize2 if nested else 0), ct.c_int(1 if nested else 0), out)
    p = dict(zip(FIELDS, out))
    p["nested"] = nested
    p["ws_bytes"] = (out[13] & 0xFFFFFFFF) | (out[14] << 32)
    return p


def _b(x):
    return "true" if x else "false"


def _kernel_name(p):
    """The launched instance as a kernel trace prints it (template arguments after T)."""
    k, ns = p["kernel"], _b(p["nested"])
    if k == GEMV_TOK:
        return f"k_gemv_4bit_tok<{p['rg']}, {p['cfg']}, {ns}, {p['mt']}>"
    if k == T64:
        return f"k_gemm_4bit_t64<{ns}, 0, {p['waves'] // 4}>"
    if k == T64R:
        return f"k_gemm_4bit_t64r<{ns}>"
    if k == FEWTOK:
        return f"k_gemm_4bit_fewtok<{p['rg']}, {p['mt']}, {ns}, {_b(p['s4'])}, {p['waves']}, {_b(p['x8'])}, 0>"
    if k == WK:
        return f"k_gemm_4bit_wk<{p['mt']}, {p['waves']}, {p['rg']}, {ns}>"
    if k == SKINNY:
        return f"k_gemm_4bit_skinny<{p['mt']}, {p['rg']}, {ns}, 0, {p['waves']}>"
    if k == TILE128:
        return "k_gemm_4bit<>"
    if k == TILE256:
        return f"k_gemm_4bit_256<{_b(p['splits'] > 1)}, true, 4, false>"
    return None


def _reduce_name(p):
    if not p["reduce"]:
        return None
    if p["kernel"] == TILE256:
        return "k_splitk_reduce<>"
    return f"k_skinny_reduce<{2 if p['splits'] <= 2 else 4 if p['splits'] <= 4 else 8}>"


def _table():
    with open(GOLDEN) as f:
        return json.load(f)["rows"]


def _row_id(r):
    return f"{r['N']}x{r['K']}-rows{r['rows']}-bs{r['blocksize']}-{'nested' if r['nested'] else 'plain'}"


@pytest.mark.parametrize("row", _table(), ids=_row_id)
def test_default_plan_is_the_recorded_launch(row):
    want = row["plan"]
    p = _plan(row["N"], row["rows"], row["K"], row["blocksize"], row["blocksize2"], row["nested"])
    if row["nested"] and want["kernel"].startswith(("k_gemm_4bit<", "k_gemm_4bit_256<")):
        # only a tile kernel is left: with compressed statistics the entry returns 1 and is called again with plain ones
        assert p["kernel"] == NONE
        p = _plan(row["N"], row["rows"], row["K"], row["blocksize"], 0, False)
    assert _kernel_name(p) == want["kernel"]
    assert (p["grid"], p["threads"]) == (want["grid"], want["threads"])
    assert _reduce_name(p) == want["reduce"]
    assert p["ws_bytes"] <= _lib().cgemm_4bit_workspace_bytes(row["N"], row["rows"], row["K"])


def test_table_covers_every_stage_and_variant_of_the_default_rule():
    """So that a stage cannot drop out of the table unnoticed: each default-reachable stage and template variant."""
    rows = _table()
    plans = [(r, r["plan"]["kernel"], r["plan"]) for r in rows]

    def has(pred):
        return any(pred(r, k, p) for r, k, p in plans)

    def args(k):
        return [a.strip() for a in k[k.index("<") + 1:-1].split(",")]

    gemv = [(r, k) for r, k, _ in plans if k.startswith("k_gemv_4bit_tok<")]
    assert {r["rows"] for r, _ in gemv} >= {2, 4} and {args(k)[3] for _, k in gemv} == {"2", "4"}
    assert all(r["N"] >= 256 for r, _ in gemv)
    assert any(r["N"] < 3057 for r, _ in gemv), "the weight too narrow for the whole-K MFMA kernel"
    assert any(r["N"] > 12288 for r, _ in gemv), "four row groups per workgroup: the MFMA kernel declines 2..4 rows"
    ft = [args(k) for _, k, _ in plans if k.startswith("k_gemm_4bit_fewtok<")]      # RG, MT, NESTED, S4, WAVES, X8, ABL
    assert {a[0] for a in ft} == {"1", "2", "3", "4"}
    assert {(a[1], a[5]) for a in ft} == {("1", "true"), ("1", "false"), ("2", "false")}
    assert {a[3] for a in ft} == {"true", "false"}
    assert ["3", "2", "true", "false", "4", "false", "0"] in ft or ["3", "2", "false", "false", "4", "false", "0"] in ft
    assert has(lambda r, k, p: k.startswith("k_gemm_4bit_wk<") and r["rows"] <= 6 and 64 <= (r["N"] + 15) // 16 < 512)
    sk = [(args(k), p) for _, k, p in plans if k.startswith("k_gemm_4bit_skinny<")]  # MT, NB, NESTED, ABL, W
    assert {a[0] for a, _ in sk} == {"1", "2", "4"}
    assert {p["reduce"] is not None for _, p in sk} == {True, False}
    assert {(a[1], a[4]) for a, _ in sk if a[0] == "4"} == {("3", "4"), ("6", "8")}, "cfg 0 and cfg 2"
    t64 = [(args(k), p) for _, k, p in plans if k.startswith("k_gemm_4bit_t64<")]    # NESTED, ABL, KP
    assert {a[2] for a, _ in t64} == {"1", "2"}
    assert {p["reduce"] is not None for _, p in t64} == {True, False}
    assert has(lambda r, k, p: r["nested"] and r["K"] % 128 != 0 and r["N"] < 3057 and k.startswith("k_gemm_4bit_256<"))
    assert has(lambda r, k, p: k == "k_gemm_4bit<>")
    assert has(lambda r, k, p: k.startswith("k_gemm_4bit_256<false"))
    assert has(lambda r, k, p: k.startswith("k_gemm_4bit_256<true") and p["reduce"] == "k_splitk_reduce<>")


class _Knobs:
    """Set knobs through their setters for one block, then back to the defaults."""
    DEFAULTS = {"cgemm_4bit_set_fewtoken_kernel": 0, "cgemm_4bit_set_skinny_config": -1, "cgemm_4bit_set_fewtok_mode": 0,
                "cgemm_4bit_set_t64_mode": 0, "cgemm_4bit_set_t64_waves": 0, "cgemm_4bit_set_t64_regfed": 1,
                "cgemm_4bit_set_tile": 0}

    def __init__(self, **kw):
        self.kw = {"cgemm_4bit_set_" + k: v for k, v in kw.items()}

    def __enter__(self):
        for name, v in self.kw.items():
            getattr(_lib(), name)(ct.c_int(v))

    def __exit__(self, *exc):
        for name in self.kw:
            getattr(_lib(), name)(ct.c_int(self.DEFAULTS[name]))


# (rows, N, K) of tests/test_matmul4bit_gpu.py::test_fewtoken_whole_k_and_split_k_kernels
WK_SHAPES = [(5, 1001, 2048), (8, 11008, 4096), (16, 4096, 11008), (24, 4099, 4096), (32, 1, 256), (7, 300, 128),
             (17, 4096, 4096), (12, 28672 // 8, 8192)]
# ... ::test_fewtoken_split_k_geometries
SKINNY_SHAPES = [(40, 1001, 2048), (64, 4096, 11008), (33, 4099, 4096), (12, 300, 1152), (24, 130, 256), (64, 129, 128),
                 (48, 1024, 8192)]
# ... ::test_gemm_4bit_multirow_gemv_matches_gemv (N, K), 2..4 rows
GEMV_SHAPES = [(11008, 4096), (4096, 11008), (4096, 4096), (1001, 2048), (63, 128), (28672, 1024), (3584, 8192),
               (40000, 4096)]
# ... ::test_fewtok32_kernel_vs_oracle
FEWTOK_SHAPES = [(1, 4096, 4096), (2, 11008, 4096), (5, 1001, 2048), (8, 4096, 11008), (13, 300, 1152), (16, 8192, 256),
                 (17, 520, 640), (32, 11008, 4096), (31, 63, 11008), (3, 14336, 4096), (24, 14337, 1024), (9, 8200, 768)]
# tests/test_t64_gpu.py::test_t64_vs_oracle (rows, N, K), t64 mode
T64_SHAPES = [((33, 11008, 4096), 0), ((64, 11008, 4096), 0), ((48, 4096, 11008), 0), ((64, 4096, 4096), 0),
              ((40, 1000, 2304), 0), ((64, 193, 256), 0), ((57, 3584, 8192), 0), ((1, 4096, 4096), 2),
              ((17, 520, 768), 2), ((64, 28672, 512), 0)]
# tests/test_matmul4bit_gpu.py::test_gemm_4bit_each_tile_kernel
TILE_SHAPES = [(256, 256, 128), (300, 520, 640), (1000, 384, 256)]


@pytest.mark.parametrize("nested", [False, True])
def test_forced_fewtoken_kernel(nested):
    for rows, N, K in WK_SHAPES:
        with _Knobs(fewtoken_kernel=2):
            p = _plan(N, rows, K, nested=nested)
            assert p["kernel"] == WK and p["mt"] == (1 if rows <= 16 else 2), (rows, N, K)
            assert p["waves"] == (4 if (N + 15) // 16 >= 512 else 8)
        with _Knobs(fewtoken_kernel=1):
            assert _plan(N, rows, K, nested=nested)["kernel"] == SKINNY, (rows, N, K)


@pytest.mark.parametrize("nested", [False, True])
@pytest.mark.parametrize("cfg", [0, 1, 2])
def test_forced_skinny_config(nested, cfg):
    for rows, N, K in SKINNY_SHAPES:
        with _Knobs(fewtoken_kernel=1, skinny_config=cfg):
            p = _plan(N, rows, K, nested=nested)
        mt = 1 if rows <= 16 else 2 if rows <= 32 else 4
        nb = {1: 10, 2: 5, 4: 3}[mt] * (2 if cfg == 2 else 1)
        assert (p["kernel"], p["cfg"], p["mt"], p["rg"], p["waves"]) == (SKINNY, cfg, mt, nb, 4 if cfg == 0 else 8)
        assert p["splits"] == (K // 128 + nb - 1) // nb and p["reduce"] == (p["splits"] > 1)
        assert p["grid"] == (N + 16 * p["waves"] - 1) // (16 * p["waves"]) * p["splits"]


@pytest.mark.parametrize("nested", [False, True])
def test_forced_fewtok_mode(nested):
    for N, K in GEMV_SHAPES:
        for rows in (2, 3, 4):
            with _Knobs(fewtok_mode=1):                 # the whole-K MFMA kernel off: the multi-row GEMV itself
                p = _plan(N, rows, K, nested=nested)
            assert (p["kernel"] == GEMV_TOK) == (N >= 256), (rows, N, K)
            if N >= 256:
                assert p["mt"] == (2 if rows == 2 else 4)
    for bs in (64, 256):
        for rows, N, K in FEWTOK_SHAPES:
            with _Knobs(fewtok_mode=2):
                p = _plan(N, rows, K, blocksize=bs, nested=nested)
            assert p["kernel"] == FEWTOK, (rows, N, K, bs)
            assert p["mt"] == (1 if rows <= 16 else 2) and p["rg"] == min(4, max(1, (N + 4095) // 4096))
            assert p["s4"] == (bs == 64 and K % 256 == 0) and p["x8"] == (rows <= 8)


@pytest.mark.parametrize("nested", [False, True])
@pytest.mark.parametrize("waves", [1, 2])
def test_forced_t64_mode_and_waves(nested, waves):
    for (rows, N, K), mode in T64_SHAPES:
        with _Knobs(t64_mode=mode, t64_waves=waves, fewtok_mode=1):
            p = _plan(N, rows, K, nested=nested)
        assert p["kernel"] == T64 and p["waves"] == 4 * waves, (rows, N, K)
        assert p["grid"] == (N + 191) // 192 * p["splits"] and p["reduce"] == (p["splits"] > 1)
        with _Knobs(t64_mode=mode, t64_regfed=2, fewtok_mode=1):
            assert _plan(N, rows, K, nested=nested)["kernel"] == T64R
        with _Knobs(t64_mode=1, fewtok_mode=1):
            assert _plan(N, rows, K, nested=nested)["kernel"] in (WK, SKINNY, GEMV_TOK)
        with _Knobs(t64_mode=mode, fewtok_mode=1):
            assert _plan(N, rows, K, blocksize=256, nested=nested)["kernel"] != T64     # blocksize 64 only


@pytest.mark.parametrize("tile", [128, 256])
def test_forced_tile(tile):
    for rows, N, K in TILE_SHAPES + [(3, 512, 1024), (16, 1024, 2048)]:
        with _Knobs(tile=tile):
            assert _plan(N, rows, K, nested=False)["kernel"] == (TILE128 if tile == 128 else TILE256), (rows, N, K)
            assert _plan(N, rows, K, nested=True)["kernel"] == NONE      # the tile kernels need plain statistics


def test_bad_arguments_and_declines():
    assert _plan(512, 8, 96, nested=False)["kernel"] == BAD_ARGS        # K % 64 != 0
    assert _plan(512, 8, 320, nested=True)["kernel"] == NONE
    assert _plan(512, 65, 1024, nested=True)["kernel"] == NONE          # more than 64 rows: no few-token kernel
