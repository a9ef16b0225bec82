"""GPU: the GroupNorm and LayerNorm kernels (csrc/norm.hip) to the bit.

1. Against tests/golden/norm_bits.json: the sha256 of every output of tests/norm_cases.py as the commit named in the fixture wrote it (inputs
   built from integer arithmetic; the GroupNorm statistics of these inputs are exact in fp32, so chunking and CU count do not enter).
2. The identity csrc/norm.hip promises for the second output of layer_norm_add_table, which needs no fixture: y is what odise_hip_layer_norm
   writes and y2 = y + table[row % P] is what add_vec_table_kernel writes from that y."""
import ctypes as C

import numpy as np
import pytest

import norm_cases as N
from odise_amd import _lib

pytestmark = pytest.mark.gpu

CASES = N.cases()


@pytest.fixture(scope="module")
def fixture():
    return N.load_fixture()


@pytest.mark.parametrize("name,run", CASES, ids=[n for n, _ in CASES])
def test_output_bits_match_the_recorded_commit(ctx, fixture, name, run):
    got = N.digest(run(ctx))
    want = fixture["cases"][name]
    assert got == want, (f"{name}: sha256 {got} != {want} recorded from commit {fixture['commit']} ({fixture['device']}, {fixture['hipcc']}).  "
                         f"A change of csrc/norm.hip that is meant to keep every bit did not.  If the compiler or the device changed instead, check out "
                         f"a commit whose norm kernels are trusted, build it there and re-record: python tests/norm_cases.py --commit <its id>")


def test_fixture_lists_exactly_the_cases(fixture):
    assert sorted(fixture["cases"]) == sorted(n for n, _ in CASES)


@pytest.mark.parametrize("rows,Cc,P", N.TABLE_CASES)
def test_layer_norm_second_output_is_add_vec_table_of_the_first(ctx, rows, Cc, P):
    x = ctx.to_device(N.ln_input(rows, Cc))
    g, b = (ctx.to_device(t) for t in N.gamma_beta(Cc))
    tab = ctx.to_device(N.table(P, Cc))
    y, y2, want2 = (ctx.empty((rows, Cc), np.float16) for _ in range(3))
    _lib.check(ctx.lib.odise_hip_layer_norm_table(ctx.h, x, y, g, b, rows, Cc, C.c_float(1e-5), y2, tab, P), "layer_norm_table")
    plain = ctx.layer_norm(x, g, b, 1e-5)
    assert np.array_equal(y.numpy(), plain.numpy()), "the first output differs from odise_hip_layer_norm's"
    assert rows % P == 0
    _lib.check(ctx.lib.odise_hip_add_vec_table(ctx.h, y, None, tab, want2, rows // P, P, Cc), "add_vec_table")
    assert np.array_equal(y2.numpy(), want2.numpy()), "the second output differs from add_vec_table(y, NULL, table)"


def test_layer_norm_second_output_is_refused_beyond_256_channels(ctx):
    rows, Cc, P = 16, 320, 4
    x = ctx.to_device(N.ln_input(rows, Cc))
    tab = ctx.to_device(N.table(P, Cc))
    y, y2 = ctx.zeros((rows, Cc), np.float16), ctx.zeros((rows, Cc), np.float16)
    rc = ctx.lib.odise_hip_layer_norm_table(ctx.h, x, y, None, None, rows, Cc, C.c_float(1e-5), y2, tab, P)
    assert rc == -1, rc      # ODISE_ERR_ARG
    ctx.sync()
    assert not y.numpy().any() and not y2.numpy().any(), "a refused call launched something"
