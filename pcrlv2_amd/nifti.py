"""A minimal NIfTI-1 reader and writer (single-file `.nii` / `.nii.gz`), in the spirit of luna_prep.read_metaimage: no nibabel.

What is read of the 348-byte header: `sizeof_hdr` (348 in one of the two byte orders decides the file's endianness), `dim`, `datatype`, `bitpix`,
`pixdim[1..3]`, `vox_offset`, `scl_slope` / `scl_inter` and `magic`.  Data types 2 (uint8), 4 (int16), 8 (int32), 16 (float32), 64 (float64),
256 (int8) and 512 (uint16).  The volume is returned in DISK order, [Z, Y, X] with x fastest -- the order pcrlv2_amd/seg_prep.py uploads.

NO reorientation: qform / sform (and every other header field) are carried in the raw header bytes and written back by `write_nifti(header=...)`,
never applied.  A case whose channels were stored in different orientations is not detected beyond its shape and spacing.

Errors are NiftiError (a ValueError) with the path in the message: a truncated file, dim[0] != 3 (trailing dimensions of 1 are allowed), an unknown
data type, NIfTI-2 (sizeof_hdr 540) and `.hdr` / `.img` pairs (magic `ni1`).
"""
from __future__ import annotations

import gzip
import struct

import numpy as np

HEADER_BYTES = 348
DTYPES = {2: "u1", 4: "i2", 8: "i4", 16: "f4", 64: "f8", 256: "i1", 512: "u2"}
CODES = {np.dtype(v).newbyteorder("=").str[1:]: k for k, v in DTYPES.items()}


class NiftiError(ValueError):
    pass


def _open(path, mode):
    return gzip.open(path, mode) if str(path).endswith(".gz") else open(path, mode)


def _write(path, payload):
    with open(path, "wb") as f:
        if str(path).endswith(".gz"):      # no file name, no time stamp in the gzip header: equal volumes give equal files
            with gzip.GzipFile(filename="", mode="wb", fileobj=f, mtime=0) as g:
                g.write(payload)
        else:
            f.write(payload)


def parse_header(raw, path="<header>"):
    """348 raw bytes -> {'endian': '<' | '>', 'shape': (X, Y, Z), 'datatype', 'spacing': (sx, sy, sz), 'vox_offset', 'slope', 'inter'}."""
    if len(raw) < HEADER_BYTES:
        raise NiftiError(f"{path}: truncated, {len(raw)} bytes where the NIfTI-1 header has {HEADER_BYTES}")
    endian = None
    for e in "<>":
        size = struct.unpack(e + "i", raw[0:4])[0]
        if size == HEADER_BYTES:
            endian = e
        elif size == 540:
            raise NiftiError(f"{path}: NIfTI-2 (sizeof_hdr 540) is not supported; convert to NIfTI-1")
    if endian is None:
        raise NiftiError(f"{path}: sizeof_hdr is neither 348 nor its byte swap: not a NIfTI-1 file")
    magic = bytes(raw[344:348])
    if magic[:3] == b"ni1":
        raise NiftiError(f"{path}: an Analyze-style .hdr / .img pair (magic 'ni1') is not supported; store a single .nii")
    if magic[:3] != b"n+1":
        raise NiftiError(f"{path}: magic {magic!r} is not 'n+1'")
    dim = struct.unpack(endian + "8h", raw[40:56])
    if dim[0] < 3 or dim[0] > 7 or any(d != 1 for d in dim[4:dim[0] + 1]) or any(d < 1 for d in dim[1:4]):
        raise NiftiError(f"{path}: dim = {dim}: a 3D volume is supported (dim[0] = 3, or more with every further dimension 1)")
    datatype = struct.unpack(endian + "h", raw[70:72])[0]
    if datatype not in DTYPES:
        raise NiftiError(f"{path}: datatype {datatype} is not one of {sorted(DTYPES)}")
    pixdim = struct.unpack(endian + "8f", raw[76:108])
    vox_offset, slope, inter = struct.unpack(endian + "3f", raw[108:120])
    spacing = tuple(abs(float(p)) if p != 0 and np.isfinite(p) else 1.0 for p in pixdim[1:4])
    return {"endian": endian, "shape": tuple(int(d) for d in dim[1:4]), "datatype": int(datatype), "spacing": spacing,
            "vox_offset": int(vox_offset) if np.isfinite(vox_offset) else 0, "slope": float(slope), "inter": float(inter)}


def scaled(h):
    """A header's scaling is applied unless it is the identity (slope 0 means 'none' in NIfTI-1)."""
    s, i = h["slope"], h["inter"]
    return not (s == 0.0 or not np.isfinite(s) or not np.isfinite(i) or (s == 1.0 and i == 0.0))


def read_nifti(path, raw_values=False):
    """-> (volume [Z, Y, X] in disk order, spacing (sx, sy, sz), header bytes).  The volume is int16 (datatype 4 without scaling) or float32 (every
    other type: scaled in float64, rounded to float32 once); with raw_values the stored type after scaling in float64 where the header scales."""
    try:
        with _open(path, "rb") as f:
            raw = f.read(HEADER_BYTES)
            h = parse_header(raw, path)
            X, Y, Z = h["shape"]
            dt = np.dtype(h["endian"] + DTYPES[h["datatype"]])
            skip = max(h["vox_offset"], 352) - HEADER_BYTES
            if len(f.read(skip)) != skip:
                raise NiftiError(f"{path}: truncated before vox_offset {h['vox_offset']}")
            want = X * Y * Z * dt.itemsize
            buf = f.read(want)
    except (EOFError, gzip.BadGzipFile, OSError) as e:
        if isinstance(e, FileNotFoundError):
            raise
        raise NiftiError(f"{path}: {e}") from e
    if len(buf) != want:
        raise NiftiError(f"{path}: truncated, {len(buf)} data bytes where dim says {want}")
    vol = np.frombuffer(buf, dtype=dt).reshape(Z, Y, X)
    if scaled(h):
        vol = vol.astype(np.float64) * h["slope"] + h["inter"]
    else:
        vol = vol.astype(dt.newbyteorder("="), copy=False)
    if not raw_values and not (vol.dtype == np.int16):
        vol = vol.astype(np.float32)
    return vol, h["spacing"], bytes(raw)


def write_nifti(path, vol_zyx, spacing=(1.0, 1.0, 1.0), header=None, big_endian=None, slope=1.0, inter=0.0):
    """Write [Z, Y, X] (disk order) of one of the supported types.  header: 348 bytes of another file whose geometry (qform, sform, pixdim, ...) and
    byte order are kept; dim, datatype, bitpix, vox_offset, scaling and magic are rewritten."""
    vol = np.asarray(vol_zyx)
    key = vol.dtype.newbyteorder("=").str[1:]
    if vol.ndim != 3 or key not in CODES:
        raise NiftiError(f"{path}: cannot write a {vol.dtype} array of shape {vol.shape}")
    if header is not None:
        endian = parse_header(header, path)["endian"]
        hdr = bytearray(header[:HEADER_BYTES])
    else:
        endian = ">" if big_endian else "<"
        hdr = bytearray(HEADER_BYTES)
        struct.pack_into(endian + "8f", hdr, 76, 1.0, float(spacing[0]), float(spacing[1]), float(spacing[2]), 1.0, 1.0, 1.0, 1.0)
        hdr[123] = 2      # xyzt_units: millimetres
    if big_endian is not None and header is not None and (">" if big_endian else "<") != endian:
        raise NiftiError(f"{path}: the header's byte order is kept; big_endian contradicts it")
    Z, Y, X = vol.shape
    if max(X, Y, Z) > 32767:
        raise NiftiError(f"{path}: an extent above 32767 does not fit NIfTI-1's dim")
    struct.pack_into(endian + "i", hdr, 0, HEADER_BYTES)
    struct.pack_into(endian + "8h", hdr, 40, 3, X, Y, Z, 1, 1, 1, 1)
    struct.pack_into(endian + "2h", hdr, 70, CODES[key], vol.dtype.itemsize * 8)
    struct.pack_into(endian + "3f", hdr, 108, 352.0, float(slope), float(inter))
    hdr[344:348] = b"n+1\0"
    _write(path, bytes(hdr) + b"\0\0\0\0" + np.ascontiguousarray(vol, dtype=vol.dtype.newbyteorder(endian)).tobytes())
