"""decodeLDPC and calcLLR on the GPU at every row of tests/fec_shape_cases.py against the numpy restatement
(tests/fec_restatement.py, pinned to the reference's recorded results by tests/test_fec_restatement.py), at the bounds of
tests/fec_cases.py (run with -m gpu): min-sum bit-equal, NaN included and at the same places; sum-product in float64 within 1e-9
rel-L2 per codeword and 1e-9 of the column's max |ref| per element; in float32 within 4 x the restatement's own distance between
its float32 and float64 runs, per codeword; decisions, frameErrors and lastIter equal; calcLLR within 1e-9 relative (floor 1e-12).
Both engines, both orientations, numpy and DeviceArray, a second call and engine 'auto' must give the same bytes."""
import numpy as np
import pytest

import fec_cases as fc
import fec_shape_cases as fs
import opticommpy_amd as oa
from opticommpy_amd import _lib, device, fec
from test_gpu_fec import decode, same_bits

pytestmark = pytest.mark.gpu

LARGEST = {}                                                             # (group, precision) -> largest figure fs.compare returned


@pytest.mark.parametrize("row", fs.ROWS, ids=lambda r: r.id)
def test_shape_row_matches_the_restatement(row):
    fs.check_conditions(row)
    H, x = fs.graph(row.graph), fs.signals(row)
    assert _lib.fec_lds_bytes(len(H.indices), H.shape[1], row.prec) <= _lib.FEC_LDS_BUDGET
    first = decode(x, fs.param(row, engine="lds"), transposed=False, on_device=False)
    figure = fs.compare(row, first, "lds")
    if figure is not None:
        LARGEST[row.group, row.prec] = max(LARGEST.get((row.group, row.prec), 0.0), figure)
    same_bits(decode(x, fs.param(row, engine="global"), transposed=True, on_device=True), first, (row.id, "global"))
    same_bits(decode(x, fs.param(row, engine="auto"), transposed=row.ncw % 2 == 0, on_device=row.ncw % 2 == 1), first, (row.id, "auto"))
    if row.group == "iter":                                              # reading the flags early changes nothing
        for every in (1, 2):
            same_bits(decode(x, fs.param(row, engine="global", syncEvery=every)), first, (row.id, "syncEvery", every))


@pytest.mark.parametrize("row", fs.LLR_ROWS, ids=lambda r: r.id)
def test_llr_shape_row_matches_the_restatement(row):
    fs.check_llr_conditions(row)
    g = fs.llr_signals(row)
    args = (g["sigma2"], g["constSymb"], g["bitMap"], g["px"])
    x0 = g["rxSymb"].copy()
    got = oa.calcLLR(x0, *args)
    assert type(got) is np.ndarray and np.array_equal(x0, g["rxSymb"])
    fs.compare_llr(row, got, "numpy")
    xd = oa.to_device(x0)
    before = device.transfer_counts()
    gd = oa.calcLLR(xd, *args)
    gd2 = oa.calcLLR(xd, *args)
    assert device.transfer_counts() == before and type(gd) is oa.DeviceArray and gd.shape == got.shape and gd.dtype == np.float64
    assert gd.get().tobytes() == got.tobytes() == gd2.get().tobytes() and np.array_equal(xd.get(), x0)
    other = np.complex64 if x0.dtype == np.complex128 else np.complex128                 # the other input type: widened on load
    assert oa.calcLLR(x0.astype(other).astype(np.complex128), *args).tobytes() == oa.calcLLR(x0.astype(other), *args).tobytes()


def test_more_graphs_than_the_cache_holds():
    """Twenty distinct small graphs in a row push the first out of the cache of device graphs (16); decoding on it again uploads it
    anew and gives the same bytes."""
    fec.release_graphs()
    assert fec.graph_cache_info() == []
    rng = np.random.default_rng(450)
    x = 2 * (1 + 0.7 * rng.normal(size=(24, 5))) / 0.49
    graphs = []
    for k in range(fec._GRAPH_CAP + 4):
        indptr, indices = fs.sampled_graph(np.random.default_rng(460 + k), 12, 24, (), 2, 6)
        graphs.append(fc.Csr(indptr, indices, (12, 24)))
    assert len({(H.indptr.tobytes(), H.indices.tobytes()) for H in graphs}) == len(graphs)
    results, keys = [], []
    for k, H in enumerate(graphs):
        results.append(decode(x, fc.Param(H=H, alg="SPA", maxIter=6, prec=np.float64, engine=("lds", "global")[k % 2])))
        keys.append(fec.graph_cache_info()[-1])                          # most recently used last
        assert len(fec.graph_cache_info()) == min(k + 1, fec._GRAPH_CAP)
    assert len(set(keys)) == len(graphs) and len({r[1].tobytes() for r in results}) > 1      # (the graphs do decode differently)
    assert fec.graph_cache_info() == keys[-fec._GRAPH_CAP:]              # the first four have been destroyed
    again = decode(x, fc.Param(H=graphs[0], alg="SPA", maxIter=6, prec=np.float64, engine="global"), transposed=True, on_device=True)
    same_bits(again, results[0], "the first graph again")
    info = fec.graph_cache_info()
    assert len(info) <= fec._GRAPH_CAP and info[-1] == keys[0] and keys[4] not in info
    same_bits(decode(x, fc.Param(H=graphs[-1], alg="SPA", maxIter=6, prec=np.float64, engine="lds")), results[-1], "the last graph again")
    fec.release_graphs()
    assert fec.graph_cache_info() == []


def test_largest_errors_per_group():
    """Prints what the rows above measured (they run first): per group the largest rel-L2 distance of a float64 sum-product
    posterior to the restatement's, and the largest multiple of the restatement's own float32 error a float32 one is away from
    its float64 run."""
    for (group, prec), figure in sorted(LARGEST.items()):
        what = "rel-L2 to the restatement" if prec == "float64" else "distance to the float64 run / the restatement's own"
        print(f"SPA {prec} {group:7s} largest {what}: {figure:.2e}")
        assert figure <= (fc.REL if prec == "float64" else fc.F32_FACTOR)
