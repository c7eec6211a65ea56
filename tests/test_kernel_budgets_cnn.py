"""The CNN kernels (csrc/cnn.hip) use no scratch and at most 64 KB of LDS per workgroup, from the compiler's own report
(the one tests/test_kernel_budgets.py reads).  Accumulator registers are allowed here: the contraction runs on the
matrix pipe.  No GPU needed: hipcc cross-compiles for gfx950."""
import pytest

from pde_opt_amd.csrc import build as B


@pytest.fixture(scope="module")
def res():
    B.build(verbose=False)
    return {k: v for k, v in B.kernel_resources().items() if k.startswith("cnn_")}


def test_every_instantiation_is_reported(res):
    # conv: 2 dtypes x (3 activations x 4 widths + the scalar epilogue); wgrad and its reduction: 2 dtypes each
    assert sum(k.startswith("cnn_conv3x3_kernel<") for k in res) == 26
    for k in ("cnn_wgrad_kernel", "cnn_wgrad_reduce_kernel"):
        assert f"{k}<float>" in res and f"{k}<double>" in res
    assert len(res) == 30


def test_cnn_kernels_use_no_scratch_and_two_workgroups_fit_a_cu(res):
    assert res
    for name, v in res.items():
        assert v["scratch"] == 0, name
        assert v["lds_static"] <= 64 * 1024, name  # 160 KB of LDS per CU: two workgroups whatever the registers
        assert v["occupancy"] >= 2, name           # and two waves per SIMD hide the matrix pipe's latency

