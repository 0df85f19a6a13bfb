"""numpy restatement of the candidate-cube definitions (include/pcrl_hip.h, `pcrl_prep_cubes`; pcrlv2_amd/luna_nodules.py), for the tests."""
import numpy as np

AIR = -1000


def cubes(vol_zyx, start, cube, float32=False):
    """vol int16 [Z, Y, X], start int [M, 3] = (x0, y0, z0) -> [M, CX, CY, CZ]: pad with air, slice, transpose to (x, y, z), clip to the HU window;
    float32: np.float32((float64(v) + 1000) / 2000)."""
    vol = np.asarray(vol_zyx, dtype=np.int16)
    start = np.asarray(start, dtype=np.int64).reshape(-1, 3)
    CX, CY, CZ = cube
    Z, Y, X = vol.shape
    # enough air on every side for any start this far out; starts further away are all air
    px, py, pz = CX + X, CY + Y, CZ + Z
    padded = np.pad(vol, ((pz, pz), (py, py), (px, px)), mode="constant", constant_values=AIR)
    out = np.empty((start.shape[0], CX, CY, CZ), dtype=np.int16)
    for m, (x0, y0, z0) in enumerate(start):
        x0, y0, z0 = (int(np.clip(v, -p, n)) for v, p, n in ((x0, px, X), (y0, py, Y), (z0, pz, Z)))      # beyond the pad: still all air
        block = padded[z0 + pz:z0 + pz + CZ, y0 + py:y0 + py + CY, x0 + px:x0 + px + CX]
        out[m] = np.clip(block.transpose(2, 1, 0), -1000, 1000)
    return unit(out) if float32 else out


def unit(v):
    return np.float32((np.asarray(v).astype(np.float64) + 1000) / 2000)


def world_to_start(world, offset, diag, cube):
    """floor(d * (world - offset) + 0.5) - cube / 2 per axis, d = the +-1 diagonal of TransformMatrix."""
    w = np.asarray(world, dtype=np.float64).reshape(-1, 3)
    vox = np.floor(np.asarray(diag, dtype=np.float64) * (w - np.asarray(offset, dtype=np.float64)) + 0.5).astype(np.int64)
    return vox - np.asarray(cube, dtype=np.int64) // 2
