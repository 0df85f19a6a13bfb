"""CPU: the convolution dispatchers' routing, pinned against the table the PARENT revision answered (tools/make_route_table.py)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_route_table_matches_parent_revision(golden_dir, monkeypatch):
    """Every int64_t / size_t query of the 3D conv, composed up-conv, transposed-conv, to-1, c1, 2D conv and stem families -- kernel kinds, statistics
    rows, workspace sizes: what the Python side allocates by -- for the layer shapes of C2, C4 and the 2D step plus awkward shapes (W % 16 != 0, D % 4 != 0,
    96 channels, degenerate extents, channel counts no kernel takes), both dtypes, under every test-hook setting, equals tests/golden/route_table.npz.
    That fixture was written from a build of the parent commit (PCRL_LIB), not from this code; a deliberate routing change regenerates it the same way."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_route_table as T
    from pcrlv2_amd import _lib
    for k in T.ENV_SWITCHES:       # the table holds the switches' defaults (the library reads them once per process, on first use)
        monkeypatch.delenv(k, raising=False)
    fx = np.load(os.path.join(golden_dir, "route_table.npz"))
    q = T.cases()
    assert np.array_equal(fx["digest"], T.case_digest(q)), "tools/make_route_table.py's case list changed: regenerate the fixture from the parent revision"
    assert [tuple(int(v) for v in s) for s in fx["settings"]] == T.settings()
    if not os.path.exists(_lib.LIBPATH):
        import __graft_entry__ as g
        g.build()
    L = _lib.lib()
    try:
        got = T.evaluate(L, q)
    finally:
        T.reset_hooks(L)
    bad = np.argwhere(got != fx["table"])
    assert len(bad) == 0, [(T.settings()[i], q[j], int(fx["table"][i, j]), int(got[i, j])) for i, j in bad[:10]]
    assert len(q) > 5000 and (fx["table"] != fx["table"][0]).any(axis=0).sum() > 500        # the hooks do move routes in the table
