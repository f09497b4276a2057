"""Which kernel a shape takes: the host-only route functions (mdt_policy_amd/csrc/mdt_route.h, mdt_route_train.h) against the
committed table.

tests/c_client/route_table.cpp is a stand-alone program over the route header: no GPU, no library, nothing loaded into Python.  It is
built with the address and undefined-behaviour sanitizers and its lines are compared, key by key, with
tests/c_client/route_table.expected -- the kernel name with its template integers, grid, threads and dynamic LDS bytes of every
GEMM case (each pair of cases straddles one rule of mdt_route_gemm), and the attention / MLP forms of a block at the batch sizes
where they change.  The expected GEMM lines are the kernel-trace rows of the commit before the routes moved into the header
(profiles/route_equivalence.txt); a pull request that moves a threshold changes this table on purpose or not at all.

The training path's lines -- lin_bwd/ (the Linear backward's plan: path, kernel, grid, threads, LDS, slices S of L rows, scratch
floats), attn_train/, ln/, colsum/, narrow/ -- are likewise those of the commit before mdt_route_train.h
(profiles/train_route_equivalence.txt), and the program sweeps the plan's invariants (slices cover the rows, scratch regions
disjoint and inside the total, every total inside the allocation bound of any larger capacity) into one `invariants` line.

The deep/ lines are whole training steps: every forward product, Linear backward plan and input-gradient product, on encoder and on
decoder rows, of each (configuration, batch) of tests/deep_row_configs.py.  The assertions at the end of this file name the route each
of those batches is there for, so that tests/test_gpu_deep_row_training.py cannot drift off the kernels it means to run."""
import os
import re
import shutil
import subprocess

import pytest

from tests.linear_bwd_shapes import SMALL_SHAPES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c_client", "route_table.cpp")
EXPECTED = os.path.join(ROOT, "tests", "c_client", "route_table.expected")
LDS_MAX = 160 * 1024  # bytes of LDS a workgroup can have on gfx950


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ not found: the route table program is plain C++17 and needs only a host compiler")
    exe = str(tmp_path_factory.mktemp("route") / "route_table")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    f"-I{os.path.join(ROOT, 'include')}", f"-I{os.path.join(ROOT, 'mdt_policy_amd', 'csrc')}", SRC, "-o", exe],
                   check=True, capture_output=True, text=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True)
    assert out.stderr == "", out.stderr  # a sanitizer report
    return _parse(out.stdout)


def _parse(text):
    rows = {}
    for line in text.splitlines():
        if not line.strip() or line.startswith("#"):
            continue
        key, _, val = line.partition(": ")
        assert key not in rows, f"duplicate key {key}"
        rows[key] = val
    return rows


def test_every_route_is_the_committed_one(table):
    with open(EXPECTED) as f:
        want = _parse(f.read())
    assert list(table) == list(want), "the program's cases and the committed table's differ (same keys, same order)"
    wrong = {k: (table[k], want[k]) for k in want if table[k] != want[k]}
    assert not wrong, "\n".join(f"{k}: got {g!r}, committed {w!r}" for k, (g, w) in wrong.items())


def test_no_route_asks_for_more_lds_than_a_workgroup_has(table):
    gemm = {k: v for k, v in table.items() if k.startswith("gemm/")}
    assert len(gemm) >= 60
    for key, val in gemm.items():
        if val == "REFUSED":
            continue
        m = re.fullmatch(r"k_\w+(<[^>]*>)? grid=\((\d+),(\d+),(\d+)\) threads=(\d+) lds=(\d+)", val)
        assert m, f"{key}: {val!r}"
        assert int(m.group(6)) <= LDS_MAX, f"{key}: {val}"
        assert 64 <= int(m.group(5)) <= 1024 and int(m.group(2)) >= 1, f"{key}: {val}"
    train = {k: v for k, v in table.items() if k.startswith(("lin_bwd/", "attn_train/")) and v != "REFUSED" and not v.startswith("copy ")}
    assert len(train) >= 60
    for key, val in train.items():
        m = re.search(r" grid=\((B|\d+),(\d+)(,\d+)?\) threads=(\d+) lds=(\d+)", val)
        assert m, f"{key}: {val!r}"
        assert int(m.group(5)) <= LDS_MAX and 64 <= int(m.group(4)) <= 1024 and int(m.group(2)) >= 1, f"{key}: {val}"


def test_the_plans_slices_are_the_hand_worked_ones(table):
    """S of every (M, N, K, S) of tests/linear_bwd_shapes.py -- worked out by hand, and read back off the scratch on a GPU by
    tests/test_gpu_linear_bwd.py -- is the S of the plan."""
    assert len(SMALL_SHAPES) == 21
    for M, N, K, S in SMALL_SHAPES:
        val = table[f"lin_bwd/{M}x{N}x{K}"]
        assert val.startswith("tn k_gemm_tn<") and re.search(rf" grid=\(\d+,1,{S}\) .* S={S} L=\d+ ", val), f"{M} x {N} x {K}: {S} slices by hand, {val}"


def test_the_plans_invariants_hold_over_the_sweep(table):
    assert table["invariants"].startswith("OK ("), table["invariants"]


def test_the_table_agrees_with_the_outcomes_the_rules_comments_name(table):
    # "M = 10240: N = 384 -> 8 waves, N = 1152 / 1536 -> 12 waves" (ws_shape)
    assert "k_gemm_ws<24, 1, 8, 0>" in table["gemm/10240x384_ws_split0"]
    assert "k_gemm_ws<24, 1, 12, 0>" in table["gemm/10240x1152_ws_split0"]
    assert "k_gemm_ws<24, 1, 12, 0>" in table["gemm/10240x1536_ws_split0"]
    # "1280 x 1536 -- 320 tiles -- ... stays" on the half-height tiles; 1024 x 1536 and 1280 x 1152 take the 32 x 192 tiles
    assert table["gemm/ln_1280x1536"].startswith("k_gemm<1, 1, 4,")
    assert table["gemm/ln_1024x1536"].startswith("k_gemm<2, 3, 4,") and table["gemm/ln_1280x1152"].startswith("k_gemm<2, 3, 4,")
    # the tiled attention form up to 256 tiles: "B > 272" keeps the plain projection
    assert "dec_attn=ATTN_PROJ_WIDE " in table["block/B272_no_fold"] and "dec_attn=ATTN_PLAIN " in table["block/B273_no_fold"]
    # 8192 rows: "n-tile ... else 128 wide where N is a multiple of 128, else 64" and the bf16 split kernel "from 8192 rows on"
    assert table["lin_bwd/8191x384x384"].startswith("tn k_gemm_tn<2, 1>") and table["lin_bwd/8192x384x384"].startswith("tn_split k_gemm_tn_split<2, 2>")
    # "192 wide ... for matrices of at least 576 x 192", "ONE round of them": 8 tiles x 32 slices
    assert table["lin_bwd/8192x192x768_tn_split0"].startswith("tn k_gemm_tn<3, 3>") and table["lin_bwd/8192x192x192_tn_split0"].startswith("tn k_gemm_tn<3, 1>")
    assert " grid=(8,1,32) " in table["lin_bwd/104448x1536x192_tn_split0"]
    # "170 = 510 of the 512 that are resident at once" (192 x 192 at M = 104448, fp32) is the split form's bound: never more slices
    assert int(re.search(r" S=(\d+) ", table["lin_bwd/104448x192x192"]).group(1)) <= 170
    # head groups 4 / 2 / 1; RoPE: one wave per head; rows a wave keeps in flight 1 / 2 / 2 / 3
    assert [table[f"attn_train/hd64_H{h}_fwd"].split(">")[0][-1] for h in (8, 6, 7)] == ["4", "2", "1"]
    assert table["attn_train/hd64_H8_rope_bwd"].startswith("k_attn_bwd<64> ")
    assert [re.search(r"bwd=VEC4 rb=(\d)", table[f"ln/D384_rps{r}"]).group(1) for r in (4, 5, 8, 9)] == ["1", "2", "2", "3"]
    # B = 77 is the first batch of the pair MLP (770 rows)
    assert " mlp=MLP_TWO_GEMMS " in table["block/B76"] and " mlp=MLP_FUSED_PAIR " in table["block/B77"]


# the GEMM geometries of mdt_op_set_gemm_geometry as the route text names them
GEO5, GEO9 = " k_gemm<2, 2, 4, ", " k_gemm<2, 3, 4, "   # 4 waves 32 x 128, 4 waves 32 x 192


def _deep(table, name, B, layer, tag=""):
    return table[f"deep/{name}_B{B}{tag}/{layer}"]


def test_every_deep_row_step_has_its_lines(table):
    """The deep/ lines are the steps of tests/deep_row_configs.py, batch by batch, at the rows the configurations give."""
    from tests.deep_row_configs import DEEP_DROPOUT, DEEP_REUSE, DEEP_SPLIT_OFF, DEEP_STEPS, rows_of
    assert DEEP_DROPOUT in DEEP_STEPS and DEEP_SPLIT_OFF in DEEP_STEPS and DEEP_REUSE[:2] in DEEP_STEPS
    for name, B in DEEP_STEPS + [(DEEP_REUSE[0], DEEP_REUSE[2])]:
        Me, Md = rows_of(name, B)
        assert _deep(table, name, B, "enc.qkv.fwd").startswith(f"{Me}x") and _deep(table, name, B, "dec.qkv.bwd").startswith(f"{Md}x"), (name, B)
        assert f" rows={Md} " in _deep(table, name, B, "narrow")
        assert "REFUSED" not in "".join(v for k, v in table.items() if k.startswith(f"deep/{name}_B{B}/")), (name, B)


def test_the_deep_row_batches_reach_the_routes_they_are_there_for(table):
    # geometries 5 and 9 at 4096 rows (d = 256: c_proj with its deep K on the 32 x 128 tiles, qkv on the 32 x 192 ones) ...
    assert _deep(table, "ta64_a64_d256", 64, "dec.c_proj.fwd").startswith("4096x256x1024" + GEO5)
    assert _deep(table, "ta64_a64_d256", 64, "dec.qkv.fwd").startswith("4096x768x256" + GEO9)
    # ... geometry 9 at 4096 rows of the shipped width, where geometry 5 starts at 5120 rows
    assert _deep(table, "ta64_a64", 64, "dec.qkv.fwd").startswith("4096x1152x384" + GEO9) and _deep(table, "ta64_a64", 64, "dec.c_fc.fwd").startswith("4096x1536x384" + GEO9)
    assert _deep(table, "ta64_a64", 80, "dec.c_proj.fwd").startswith("5120x384x1536" + GEO5)
    # B = 127 is the last batch below the 8192-row routes: tiled kernels, k_gemm_tn on its 64-wide tiles
    for layer in ("qkv", "proj", "c_fc", "c_proj"):
        for kind in ("fwd", "dx"):
            assert " k_gemm<" in _deep(table, "ta64_a64", 127, f"dec.{layer}.{kind}"), (layer, kind)
        assert " tn k_gemm_tn<2, 1> " in _deep(table, "ta64_a64", 127, f"dec.{layer}.bwd"), layer
    # the tall body
    assert _deep(table, "ta64_a64", 128, "dec.c_proj.fwd").startswith("8192x384x1536 k_gemm_tall<")
    assert _deep(table, "ta64_a64", 128, "dec.qkv.dx").startswith("8192x384x1152 k_gemm_tall<")
    assert _deep(table, "ctx64", 128, "enc.c_proj.fwd").startswith("8192x384x1536 k_gemm_tall<")
    assert _deep(table, "mdt_ta40", 205, "dec.qkv.fwd").startswith("8200x1536x512 k_gemm_tall<")
    # k_gemm_ws at K = 384: the fp32 body with the split forms off
    for layer in ("qkv.fwd", "proj.fwd", "c_fc.fwd", "c_proj.dx"):
        assert " k_gemm_ws<24, " in _deep(table, "ta64_a64", 128, f"dec.{layer}", "_split0"), layer
    # k_gemm_ws at K = 192
    assert " k_gemm_ws_split<12, " in _deep(table, "ta64_a64_d192", 128, "dec.qkv.fwd") and " k_gemm_ws_split<12, " in _deep(table, "ta64_a64_d192", 128, "dec.proj.fwd")
    # the split form of k_gemm_ws, on decoder and on encoder rows
    for name, side in (("ta64_a64", "dec"), ("ctx64", "enc")):
        for layer in ("qkv.fwd", "proj.fwd", "c_fc.fwd", "c_proj.dx"):
            assert " k_gemm_ws_split<24, " in _deep(table, name, 128, f"{side}.{layer}"), (name, layer)
    assert " k_gemm_ws_split<24, " in _deep(table, "ctx64", 128, "enc.kv_all.fwd")
    # k_gemm_tn_split, and its 192 x 128 tile at N = 192
    for layer in ("qkv", "proj", "c_fc", "c_proj"):
        assert " tn_split k_gemm_tn_split<2, 2> " in _deep(table, "ta64_a64", 128, f"dec.{layer}.bwd"), layer
    assert " tn_split k_gemm_tn_split<4, 3> " in _deep(table, "ta64_a64_d192", 128, "dec.proj.bwd")
    assert " tn_split k_gemm_tn_split<4, 3> " in _deep(table, "ta64_a64_d192", 128, "dec.c_proj.bwd")
    # k_gemm_tn<3, ...>: the 192-wide fp32 tiles with the split forms off
    for layer in ("qkv", "proj", "c_fc", "c_proj"):
        assert " tn k_gemm_tn<3, 3> " in _deep(table, "ta64_a64", 128, f"dec.{layer}.bwd", "_split0"), layer
    # chunk attention in those steps; the 64-token context's cross-attention stages the 10 visible keys
    assert " dec 64x64 k_attn_chunk_bwd<48, false> " in _deep(table, "ta64_a64", 128, "attn.bwd")
    assert "enc 64x64 k_attn_chunk_fwd<48, false> " in _deep(table, "ctx64", 128, "attn.fwd") and " cross 10x64 kv_rows=10 k_attn_chunk_bwd<48, false> " in _deep(table, "ctx64", 128, "attn.bwd")
    # the narrow gradients' slices of 5 and 6 rows, in the wide form (4 and 2 column tiles)
    assert _deep(table, "a64_rows2600", 260, "narrow") == "A=64 rows=2600 slice_rows=5..6 tiles=4"
    assert _deep(table, "a17_mlp_proprio_rows2600", 260, "narrow") == "A=17 rows=2600 slice_rows=5..6 tiles=2"
    assert _deep(table, "a17_mlp_proprio_rows2600", 260, "dec.head0.bwd").startswith("2600x112x384 ")


def test_the_scratch_reuse_batch_has_more_slices_than_the_capacity_batch(table):
    """tests/test_gpu_deep_row_training.py steps one model at B = 128 and at B = 105: the 384 x 384 weight gradients of the smaller
    batch are cut into more slices and need more scratch than those of the capacity batch, inside the bound sized at 8192 rows."""
    from tests.deep_row_configs import DEEP_REUSE
    name, cap, small = DEEP_REUSE
    m = re.fullmatch(r"B=(\d+) rows=(\d+) S=(\d+) total=(\d+) \| B=(\d+) rows=(\d+) S=(\d+) total=(\d+) \| bound_at_8192=(\d+)", table["deep/scratch_reuse"])
    assert m, table["deep/scratch_reuse"]
    b0, r0, s0, t0, b1, r1, s1, t1, bound = map(int, m.groups())
    assert (b0, b1) == (small, cap) and r0 < r1 == 8192
    assert s0 > s1 and t1 < t0 <= bound
    assert f" S={s0} " in _deep(table, name, small, "dec.proj.bwd") and f" S={s1} " in _deep(table, name, cap, "dec.proj.bwd")
