"""circom_compat_amd -- MI355X-native Groth16 (BN254) proving path for Circom circuits.

Host-side mirror (Python harness flavour) of the reference's surface for the proving path:

    reference (ark-circom 0.5)                              here
    ------------------------------------------------------  -----------------------------------
    read_zkey(reader) -> (ProvingKey, ConstraintMatrices)   read_zkey(path | bytes)
        src/zkey.rs:53-60
    R1CSFile::new(reader), R1CS::from(file)                 R1CSFile(path | bytes), R1CS.from_file
        src/circom/r1cs_reader.rs:26-39,54-146
    CircomCircuit{r1cs, witness}.get_public_inputs()        CircomCircuit(...).get_public_inputs()
        src/circom/circuit.rs:12-26
    CircomReduction::witness_map_from_matrices              CircomReduction.witness_map_from_matrices
        src/circom/qap.rs:23-88
    Groth16::<Bn254,CircomReduction>::                      Groth16.create_proof_with_reduction_and_matrices
        create_proof_with_reduction_and_matrices            (same argument order)
        benches/groth16.rs:52-60, src/zkey.rs:903-911
    Groth16::prove(&pk, circuit, rng)  src/zkey.rs:866      Groth16.prove(pk, matrices, circuit, rng)

All arithmetic happens in libg16_amd.so (hand-written HIP for gfx950) behind the C ABI of
include/g16_amd.h.  Witness generation (circom WASM) and the arkworks ConstraintSystem layer are out of
scope; snarkjs JSON and the Ethereum forms (reference src/ethereum.rs) are in snarkjs.py,
the command line in __main__.py.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os
import random
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _binding as B
from ._binding import G16Error, SerializationError, SynthesisError  # noqa: F401

__all__ = ["read_zkey", "R1CSFile", "R1CS", "CircomCircuit", "CircomBuilder", "CircomReduction", "LibsnarkReduction", "Groth16",
           "Prover", "ProvingKey", "VerifyingKey", "ConstraintMatrices", "Proof", "G16Error",
           "SynthesisError", "SerializationError", "fr_from_ints", "fr_to_ints", "read_wtns",
           "trapdoor_setup", "Csr", "write_zkey", "device_tensor", "verify_batch", "verify_aggregate",
           "verify_batch_fast", "verify_aggregate_keys", "verify_batch_keys", "verify_batch_fast_keys", "check_key", "KeyReport", "contribute_key", "check_contribution",
           "ContributionReport", "Srs", "trapdoor_srs", "setup_from_srs", "check_key_circuit",
           "CircuitBindingReport", "read_ptau", "write_ptau", "check_srs", "SrsReport", "contribute_srs", "new_srs",
           "LagrangeSrs", "LagrangeReport", "prepare_phase2", "prepare_phase2_times", "check_lagrange",
           "points_from_ark", "points_to_ark", "read_ark_key", "write_ark_key", "read_ark_vk", "write_ark_vk",
           "proofs_from_ark", "proofs_to_ark", "ark_point_bytes", "rerandomize", "rerandomize_keys",
           "rerandomize_times", "PreparedVerifyingKey", "prepare_verifying_key", "verify_prepared", "pairing_check",
           "verify_prepared_times", "Witness", "open_wtns", "write_wtns", "fr_from_canonical", "fr_from_canonical_times", "read_proof_json",
           "write_proof_json", "read_public_json", "write_public_json", "read_vk_json", "write_vk_json",
           "inputs_to_eth", "solidity_calldata", "GT", "gt_multiexp", "gt_from_ark", "gt_times", "pairing_products",
           "pairing", "prepare_inputs", "verify_prepared_inputs", "MsmBases", "msm", "poly_divide_linear", "KzgKey",
           "kzg_verify", "kzg_times"]

FR_MODULUS = 21888242871839275222246405745257275088548364400416034343698204186575808495617


def _np_ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _view(ptr, count, width):
    """count x width bytes of library-owned memory as a (count, width) uint8 array, without a copy"""
    if count == 0:
        return np.zeros((0, width), dtype=np.uint8)
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(count * width,)).reshape(count, width)


def _rho_array(rho, n, what):
    """the coefficients of a small-exponent test for the C ABI: None (the library draws them) or n ints in
    [0, 2^128) -> None or an (n, 2) uint64 array, low word first; `what`: the message when the count is wrong.
    Zero is refused by the library."""
    if rho is None:
        return None
    rho = [int(x) for x in rho]
    if len(rho) != n:
        raise G16Error(B.G16_ERR_INVALID, what)
    if any(not 0 <= x < 1 << 128 for x in rho):
        raise G16Error(B.G16_ERR_INVALID, "coefficients are integers in [1, 2^128)")
    return np.array([[x & 0xFFFFFFFFFFFFFFFF, x >> 64] for x in rho], dtype=np.uint64).reshape(-1, 2)


def fr_from_ints(values: Sequence[int], lib: Optional[B.Library] = None) -> np.ndarray:
    """canonical ints -> (n, 4) uint64 Montgomery limbs (the in-memory form of ark_bn254::Fr)."""
    lib = lib or B.load()
    raw = b"".join((int(v) % FR_MODULUS).to_bytes(32, "little") for v in values)
    src = np.frombuffer(raw, dtype=np.uint8)
    out = np.empty((len(values), 4), dtype=np.uint64)
    lib.check(lib.g16_fr_from_canonical(_np_ptr(src), _np_ptr(out), len(values)), loader=True)
    return out


def fr_to_ints(limbs: np.ndarray, lib: Optional[B.Library] = None) -> List[int]:
    lib = lib or B.load()
    limbs = np.ascontiguousarray(limbs, dtype=np.uint64).reshape(-1, 4)
    out = np.empty(limbs.shape[0] * 32, dtype=np.uint8)
    lib.check(lib.g16_fr_to_canonical(_np_ptr(limbs), _np_ptr(out), limbs.shape[0]), loader=True)
    b = out.tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def _as_fr(x, lib) -> np.ndarray:
    """accept Montgomery (n,4) uint64 arrays or sequences of canonical ints"""
    if isinstance(x, np.ndarray) and x.dtype == np.uint64:
        return np.ascontiguousarray(x).reshape(-1, 4)
    return fr_from_ints(list(x), lib)


class _RawDeviceBytes:
    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = {"shape": (int(nbytes),), "typestr": "|u1",
                                         "data": (int(ptr), False), "version": 2}


def device_tensor(ptr: int, nbytes: int, device=None):
    """uint8 torch view of library-owned device memory (g16_partial_buffer / g16_gather_buffer), so
    that a host framework can hand it to its collectives (RCCL all_gather) without a host copy.
    Plumbing only: torch is imported here, never by the proving path."""
    import torch
    return torch.as_tensor(_RawDeviceBytes(ptr, nbytes), device=device or "cuda")


class Csr:
    """row-major sparse rows of (coeff, index): ConstraintMatrices::{a,b} (src/zkey.rs:165-194)"""

    def __init__(self, row_ptr, col, coeff):
        self.row_ptr = np.ascontiguousarray(row_ptr, dtype=np.uint32)
        self.col = np.ascontiguousarray(col, dtype=np.uint32)
        self.coeff = np.ascontiguousarray(coeff, dtype=np.uint64).reshape(-1, 4)
        assert self.col.shape[0] == self.coeff.shape[0] == int(self.row_ptr[-1])

    @staticmethod
    def from_c(c: B.Csr, nrows: int) -> "Csr":
        nnz = int(c.nnz)
        rp = np.ctypeslib.as_array(c.row_ptr, shape=(nrows + 1,)).copy()
        col = np.ctypeslib.as_array(c.col, shape=(max(nnz, 1),))[:nnz].copy()
        co = np.ctypeslib.as_array(c.coeff, shape=(max(nnz, 1) * 4,))[:nnz * 4].copy()
        return Csr(rp, col, co)

    @staticmethod
    def from_rows(rows, lib=None) -> "Csr":
        """rows: list of lists of (coeff_int, index)"""
        rp = [0]
        col, vals = [], []
        for row in rows:
            for cf, idx in row:
                col.append(idx)
                vals.append(cf)
            rp.append(len(col))
        return Csr(rp, col, fr_from_ints(vals, lib) if vals else np.zeros((0, 4), np.uint64))

    def to_c(self) -> B.Csr:
        c = B.Csr()
        c.row_ptr = self.row_ptr.ctypes.data_as(C.POINTER(C.c_uint32))
        c.col = self.col.ctypes.data_as(C.POINTER(C.c_uint32))
        c.coeff = self.coeff.ctypes.data_as(C.POINTER(C.c_uint64))
        c.nnz = self.col.shape[0]
        return c

    @property
    def num_rows(self):
        return self.row_ptr.shape[0] - 1


class ConstraintMatrices:
    """ark_relations::r1cs::ConstraintMatrices as read_zkey fills it (src/zkey.rs:179-193)."""

    def __init__(self, num_instance_variables, num_witness_variables, num_constraints, a: Csr,
                 b: Csr):
        self.num_instance_variables = num_instance_variables
        self.num_witness_variables = num_witness_variables
        self.num_constraints = num_constraints
        self.a, self.b = a, b
        self.a_num_non_zero = a.col.shape[0]
        self.b_num_non_zero = b.col.shape[0]
        self.c_num_non_zero = 0  # src/zkey.rs:188-192: c is empty


class VerifyingKey:
    def __init__(self, alpha_g1, beta_g2, gamma_g2, delta_g2, gamma_abc_g1):
        self.alpha_g1, self.beta_g2, self.gamma_g2, self.delta_g2 = alpha_g1, beta_g2, gamma_g2, delta_g2
        self.gamma_abc_g1 = gamma_abc_g1  # (p+1, 64) uint8

    def to_eth(self, device=0, lib: Optional[B.Library] = None):
        """ethereum::VerifyingKey::as_tuple (reference src/ethereum.rs:139-161): (alpha1, beta2, gamma2, delta2, ic) as
        ints, G2 with c1 first (snarkjs.vk_to_eth)"""
        from . import snarkjs
        return snarkjs.vk_to_eth(self, device, lib)

    @staticmethod
    def from_eth(t, device=0, lib: Optional[B.Library] = None) -> "VerifyingKey":
        from . import snarkjs
        return snarkjs.vk_from_eth(t, device, lib)


class ProvingKey:
    """ark_groth16::ProvingKey<Bn254> in packed form (points: Montgomery x|y bytes)."""

    def __init__(self, n_vars, n_public, domain_size, vk: VerifyingKey, beta_g1, delta_g1, a_query,
                 b_g1_query, b_g2_query, l_query, h_query, keepalive=None):
        self.n_vars, self.n_public, self.domain_size = n_vars, n_public, domain_size
        self.vk, self.beta_g1, self.delta_g1 = vk, beta_g1, delta_g1
        self.a_query, self.b_g1_query, self.b_g2_query = a_query, b_g1_query, b_g2_query
        self.l_query, self.h_query = l_query, h_query
        self._keepalive = keepalive
        self._prover = None

    def to_c(self) -> B.KeyDesc:
        k = B.KeyDesc()
        k.n_vars, k.n_public, k.domain_size = self.n_vars, self.n_public, self.domain_size
        for name in ("a_query", "b_g1_query", "b_g2_query", "l_query", "h_query"):
            arr = getattr(self, name)
            setattr(k, name, arr.ctypes.data if arr is not None else None)
        C.memmove(k.alpha_g1, bytes(self.vk.alpha_g1), 64)
        C.memmove(k.beta_g1, bytes(self.beta_g1), 64)
        C.memmove(k.delta_g1, bytes(self.delta_g1), 64)
        C.memmove(k.beta_g2, bytes(self.vk.beta_g2), 128)
        C.memmove(k.delta_g2, bytes(self.vk.delta_g2), 128)
        return k


class _Handle:
    def __init__(self, lib, ptr, closer):
        self.lib, self.ptr, self._closer = lib, ptr, closer

    def __del__(self):
        try:
            if self.ptr:
                self._closer(self.ptr)
        except Exception:
            pass
        self.ptr = None


def read_zkey(src, lib: Optional[B.Library] = None, validate=False) -> Tuple[ProvingKey, ConstraintMatrices]:
    """read_zkey (reference src/zkey.rs:53-60): snarkjs .zkey -> (ProvingKey, ConstraintMatrices).
    validate=True runs check_key on the loaded key (on the GPU) and raises G16Error naming the first bad
    (query, index, reason) or the failed relation; the default, like the reference, looks at no point."""
    lib = lib or B.load()
    h = C.c_void_p()
    if isinstance(src, (bytes, bytearray, memoryview)):
        buf = np.frombuffer(bytes(src), dtype=np.uint8)
        lib.check(lib.g16_zkey_open_mem(_np_ptr(buf), buf.shape[0], C.byref(h)), loader=True)
    else:
        lib.check(lib.g16_zkey_open(os.fsencode(src), C.byref(h)), loader=True)
    handle = _Handle(lib, h, lib.g16_zkey_close)
    hdr = B.ZkeyHeader()
    lib.check(lib.g16_zkey_header_get(h, C.byref(hdr)), loader=True)
    kd = B.KeyDesc()
    lib.check(lib.g16_zkey_key(h, C.byref(kd)), loader=True)
    N, p, n = hdr.n_vars, hdr.n_public, hdr.domain_size

    cnt = C.c_uint32()
    icp = lib.g16_zkey_ic(h, C.byref(cnt))
    vk = VerifyingKey(bytes(hdr.alpha_g1), bytes(hdr.beta_g2), bytes(hdr.gamma_g2),
                      bytes(hdr.delta_g2), _view(icp, cnt.value, 64).copy())
    pk = ProvingKey(N, p, n, vk, bytes(hdr.beta_g1), bytes(hdr.delta_g1),
                    _view(kd.a_query, N, 64), _view(kd.b_g1_query, N, 64),
                    _view(kd.b_g2_query, N, 128), _view(kd.l_query, N - p - 1, 64),
                    _view(kd.h_query, n, 64), keepalive=handle)
    m = B.Matrices()
    lib.check(lib.g16_zkey_matrices(h, C.byref(m)), loader=True)
    mats = ConstraintMatrices(m.num_instance_variables, m.num_witness_variables, m.num_constraints,
                              Csr.from_c(m.a, m.num_constraints), Csr.from_c(m.b, m.num_constraints))
    if validate:
        rep = check_key(pk, lib=lib)
        if not rep.ok:
            raise G16Error(B.G16_ERR_INVALID, "zkey failed validation: " + rep.describe())
    return pk, mats


class R1CSFile:
    """R1CSFile::new (reference src/circom/r1cs_reader.rs:54-146)."""

    def __init__(self, src, lib: Optional[B.Library] = None):
        lib = lib or B.load()
        h = C.c_void_p()
        if isinstance(src, (bytes, bytearray, memoryview)):
            buf = np.frombuffer(bytes(src), dtype=np.uint8)
            lib.check(lib.g16_r1cs_open_mem(_np_ptr(buf), buf.shape[0], C.byref(h)), loader=True)
        else:
            lib.check(lib.g16_r1cs_open(os.fsencode(src), C.byref(h)), loader=True)
        self._handle = _Handle(lib, h, lib.g16_r1cs_close)
        hdr = B.R1csHeader()
        lib.check(lib.g16_r1cs_header_get(h, C.byref(hdr)), loader=True)
        self.version = hdr.version
        self.header = hdr
        a, b, c = B.Csr(), B.Csr(), B.Csr()
        lib.check(lib.g16_r1cs_matrices(h, C.byref(a), C.byref(b), C.byref(c)), loader=True)
        nc = hdr.n_constraints
        self.a, self.b, self.c = Csr.from_c(a, nc), Csr.from_c(b, nc), Csr.from_c(c, nc)
        cnt = C.c_uint32()
        wm = lib.g16_r1cs_wire_mapping(h, C.byref(cnt))
        self.wire_mapping = list(np.ctypeslib.as_array(C.cast(wm, C.POINTER(C.c_uint64)),
                                                       shape=(cnt.value,)))


class R1CS:
    """R1CS::from(R1CSFile) (reference src/circom/r1cs_reader.rs:26-39)."""

    def __init__(self, file: R1CSFile):
        h = file.header
        self.num_inputs = 1 + h.n_pub_in + h.n_pub_out
        self.num_variables = h.n_wires
        if self.num_inputs > self.num_variables:    # the loader refuses such a header; one built by hand gets here
            raise SerializationError(B.G16_ERR_IO, "1 + n_pub_in + n_pub_out exceeds n_wires")
        self.num_aux = self.num_variables - self.num_inputs
        self.a, self.b, self.c = file.a, file.b, file.c
        self.num_constraints = h.n_constraints
        self.wire_mapping: Optional[List[int]] = [int(x) for x in file.wire_mapping]

    @staticmethod
    def from_file(src, lib=None) -> "R1CS":
        return R1CS(R1CSFile(src, lib))

    def matrices(self) -> ConstraintMatrices:
        """A and B in the ConstraintMatrices orientation the prover consumes."""
        return ConstraintMatrices(self.num_inputs, self.num_aux, self.num_constraints, self.a, self.b)


def write_zkey(path, pk: "ProvingKey", matrices: "ConstraintMatrices", lib: Optional[B.Library] = None):
    """snarkjs-format .zkey for a key held in packed arrays (inverse of read_zkey; format notes:
    reference src/zkey.rs:1-27).  Lets synthetic keys go through the loader path."""
    lib = lib or B.load()
    kd = pk.to_c()
    a, b = matrices.a.to_c(), matrices.b.to_c()
    ic = np.ascontiguousarray(pk.vk.gamma_abc_g1, dtype=np.uint8)
    g2 = np.frombuffer(bytes(pk.vk.gamma_g2), dtype=np.uint8)
    lib.check(lib.g16_zkey_write(os.fsencode(path), C.byref(kd), _np_ptr(ic), _np_ptr(g2), C.byref(a),
                                 C.byref(b), matrices.num_constraints), loader=True)


def read_wtns(src, lib: Optional[B.Library] = None) -> np.ndarray:
    """snarkjs .wtns -> (n, 4) uint64 Montgomery witness."""
    lib = lib or B.load()
    out = C.c_void_p()
    n = C.c_uint32()
    if isinstance(src, (bytes, bytearray, memoryview)):
        buf = np.frombuffer(bytes(src), dtype=np.uint8)
        lib.check(lib.g16_wtns_read_mem(_np_ptr(buf), buf.shape[0], C.byref(out), C.byref(n)),
                  loader=True)
    else:
        lib.check(lib.g16_wtns_read(os.fsencode(src), C.byref(out), C.byref(n)), loader=True)
    arr = np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_uint64)), shape=(n.value * 4,)).copy()
    lib.g16_free(out)
    return arr.reshape(-1, 4)


class Witness:
    """A snarkjs / rapidsnark .wtns as it lies in the file (open_wtns): the header is checked, the values stay
    canonical 32-byte little-endian integers.  Prover.prove_wtns converts and range-tests them on the GPU.
    n: number of values; canonical: read-only (n, 32) uint8 view of the mapping (valid while this object lives)."""

    def __init__(self, lib, handle, n, canonical):
        self.lib, self._handle, self.n, self.canonical = lib, handle, n, canonical

    def public_inputs(self, n_public: int) -> List[int]:
        """w[1 .. n_public] as ints (converted on the host: there are few of them)"""
        if n_public + 1 > self.n:
            raise G16Error(B.G16_ERR_INVALID, f"{n_public} public inputs in a witness of {self.n} values")
        raw = self.canonical[1:1 + n_public].tobytes()
        return [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]

    def to_montgomery(self, device=0) -> np.ndarray:
        """(n, 4) uint64 Montgomery limbs, what read_wtns returns, converted on the GPU (g16_fr_convert)"""
        return fr_from_canonical(self.canonical, device=device, lib=self.lib)


def open_wtns(src, lib: Optional[B.Library] = None) -> Witness:
    """snarkjs .wtns (path or bytes) -> Witness: the file is mapped, the header checked by read_wtns' rules (and with
    its messages), nothing is converted, copied or range-tested here (g16_wtns_open)."""
    lib = lib or B.load()
    h = C.c_void_p()
    if isinstance(src, (bytes, bytearray, memoryview)):
        buf = np.frombuffer(bytes(src), dtype=np.uint8)
        lib.check(lib.g16_wtns_open_mem(_np_ptr(buf), buf.shape[0], C.byref(h)), loader=True)
    else:
        lib.check(lib.g16_wtns_open(os.fsencode(src), C.byref(h)), loader=True)
    handle = _Handle(lib, h, lib.g16_wtns_close)
    n = int(lib.g16_wtns_count(h))
    if n:
        vals = np.ctypeslib.as_array(C.cast(lib.g16_wtns_values(h), C.POINTER(C.c_uint8)), shape=(n * 32,)).reshape(n, 32)
        vals.flags.writeable = False   # the mapping is read-only
    else:
        vals = np.zeros((0, 32), dtype=np.uint8)
    return Witness(lib, handle, n, vals)


def _canonical_bytes(values) -> np.ndarray:
    """(n, 32) uint8 canonical little-endian values from such an array, raw bytes or a sequence of ints"""
    if isinstance(values, np.ndarray):
        if values.dtype != np.uint8 or values.size % 32:
            raise G16Error(B.G16_ERR_INVALID, "canonical values: a uint8 array of 32 bytes per value")
        return np.ascontiguousarray(values).reshape(-1, 32)
    if isinstance(values, (bytes, bytearray, memoryview)):
        if len(values) % 32:
            raise G16Error(B.G16_ERR_INVALID, "canonical values: 32 bytes per value")
        return np.frombuffer(bytes(values), dtype=np.uint8).reshape(-1, 32)
    try:
        raw = b"".join(int(v).to_bytes(32, "little") for v in values)
    except OverflowError:
        raise G16Error(B.G16_ERR_INVALID, "canonical values: an integer outside [0, 2^256)") from None
    return np.frombuffer(raw, dtype=np.uint8).reshape(-1, 32)


def write_wtns(path, values):
    """snarkjs .wtns, format version 2, sections 1 (n8 = 32, the bn128 prime, the count) and 2 (the values): values =
    ints, or canonical little-endian bytes as a (n, 32) uint8 array.  Nothing is reduced or range-tested."""
    v = _canonical_bytes(values)
    with open(path, "wb") as f:
        f.write(b"wtns" + (2).to_bytes(4, "little") + (2).to_bytes(4, "little"))
        f.write((1).to_bytes(4, "little") + (40).to_bytes(8, "little"))
        f.write((32).to_bytes(4, "little") + FR_MODULUS.to_bytes(32, "little") + v.shape[0].to_bytes(4, "little"))
        f.write((2).to_bytes(4, "little") + (v.shape[0] * 32).to_bytes(8, "little"))
        f.write(v.tobytes())


def fr_from_canonical(data, device=0, lib: Optional[B.Library] = None) -> np.ndarray:
    """canonical little-endian values ((n, 32) uint8 array, bytes, or ints) -> (n, 4) uint64 Montgomery limbs, converted
    on the GPU (g16_fr_convert): the bulk form of fr_from_ints.  A value >= r raises G16Error (status
    G16_ERR_INVALID) whose first_bad is the index of the first such value."""
    lib = lib or B.load()
    src = _canonical_bytes(data)
    out = np.empty((src.shape[0], 4), dtype=np.uint64)
    bad = C.c_int64(-1)
    st = lib.g16_fr_convert(device, _np_ptr(src), _np_ptr(out), src.shape[0], C.byref(bad))
    _check_canonical(lib, st, None, bad)
    return out


def _phase_times(lib, export_name, phases) -> dict:
    """the phase times behind one of the g16_..._times exports, by phase name"""
    lib = lib or B.load()
    ms = (C.c_float * len(phases))()
    lib.check(getattr(lib, export_name)(ms, len(phases)))
    return dict(zip(phases, (float(x) for x in ms)))


FR_CONVERT_PHASES = ("upload", "convert", "download")


def fr_from_canonical_times(lib: Optional[B.Library] = None) -> dict:
    """device milliseconds of this thread's last fr_from_canonical, by phase (g16_fr_convert_times)"""
    return _phase_times(lib, "g16_fr_convert_times", FR_CONVERT_PHASES)


def _check_canonical(lib, st, ctx, bad):
    try:
        lib.check(st, ctx)
    except G16Error as e:
        e.first_bad = int(bad.value)
        raise


class CircomCircuit:
    """CircomCircuit{r1cs, witness} (reference src/circom/circuit.rs:12-26).  The witness comes from
    outside (circom's WASM generator is out of scope): ints or Montgomery limbs."""

    def __init__(self, r1cs: R1CS, witness=None):
        self.r1cs = r1cs
        self.witness = witness

    def full_assignment(self):
        """The assignment CircomCircuit::generate_constraints builds (reference
        src/circom/circuit.rs:35-58): variable i takes witness[wire_mapping[i]] when the mapping is
        Some (what R1CS::from produces), witness[i] when it is None (what CircomBuilder::setup
        leaves, src/circom/builder.rs:84-85)."""
        w = self.witness
        m = getattr(self.r1cs, "wire_mapping", None)
        if w is None or m is None:
            return w
        n = self.r1cs.num_variables
        if isinstance(w, np.ndarray):
            return np.ascontiguousarray(w.reshape(-1, 4)[np.asarray(m[:n], dtype=np.int64)])
        return [w[m[i]] for i in range(n)]

    def first_unsatisfied(self, lib: Optional[B.Library] = None, device=0) -> int:
        """row index of the first constraint (A.w)(B.w) != C.w, or -1: the debug-build check of
        CircomBuilder::build (reference src/circom/builder.rs:101-114) as a GPU kernel"""
        lib = lib or B.load()
        w = _as_fr(self.full_assignment(), lib)
        a, b, c = self.r1cs.a.to_c(), self.r1cs.b.to_c(), self.r1cs.c.to_c()
        out = C.c_int64(-2)
        lib.check(lib.g16_check_satisfied(device, C.byref(a), C.byref(b), C.byref(c),
                                          self.r1cs.num_constraints, _np_ptr(w), w.shape[0],
                                          C.byref(out)))
        return int(out.value)

    def is_satisfied(self, lib: Optional[B.Library] = None) -> bool:
        return self.first_unsatisfied(lib) < 0

    def get_public_inputs(self):
        if self.witness is None:
            return None
        w = self.witness
        m = self.r1cs.wire_mapping
        if m is None:
            return [w[i] for i in range(1, self.r1cs.num_inputs)]
        return [w[m[i]] for i in range(1, self.r1cs.num_inputs)]


class CircomBuilder:
    """CircomBuilder (reference src/circom/builder.rs:60-117) minus the WASM witness calculator, which
    is out of scope: the witness comes from outside (snarkjs .wtns, JSON, another generator).  What
    it keeps is the part the proving path depends on: setup() / build() hand out circuits whose
    wire mapping is DISABLED (builder.rs:84-85), because circom witnesses are already in wire order
    -- so get_public_inputs(), the satisfiability check and Groth16.prove all read w[i]."""

    def __init__(self, r1cs: "R1CS"):
        self.r1cs = r1cs

    def setup(self) -> "CircomCircuit":
        import copy
        r = copy.copy(self.r1cs)
        r.wire_mapping = None  # "Disable the wire mapping"
        return CircomCircuit(r, None)

    def build(self, witness, sanity_check=False, lib=None) -> "CircomCircuit":
        c = self.setup()
        c.witness = witness
        if sanity_check:  # the debug_assert of builder.rs:101-114 as a kernel
            bad = c.first_unsatisfied(lib)
            if bad >= 0:
                raise G16Error(B.G16_ERR_INVALID, f"Unsatisfied constraint: {bad}")
        return c


class Proof:
    """ark_groth16::Proof<Bn254>{a, b, c} as packed affine bytes (Montgomery LE, zero = infinity)."""

    def __init__(self, raw: bytes):
        assert len(raw) == B.G16_PROOF_BYTES
        self.raw = bytes(raw)
        self.a, self.b, self.c = self.raw[:64], self.raw[64:192], self.raw[192:]

    def __eq__(self, o):
        return isinstance(o, Proof) and o.raw == self.raw

    def __repr__(self):
        return f"Proof({self.raw.hex()[:32]}...)"

    def to_ark(self, compressed=True, device=0, lib: Optional[B.Library] = None) -> bytes:
        """Proof::serialize_compressed / serialize_uncompressed: 128 / 256 bytes (g16_ark_proofs_write)."""
        return proofs_to_ark([self], compressed=compressed, device=device, lib=lib)

    @staticmethod
    def from_ark(raw, compressed=True, validate=True, device=0, lib: Optional[B.Library] = None) -> "Proof":
        """Proof::deserialize_compressed / _uncompressed of one proof (g16_ark_proofs_read)."""
        return proofs_from_ark(raw, 1, compressed=compressed, validate=validate, device=device, lib=lib)[0]

    def to_json(self, device=0, lib: Optional[B.Library] = None) -> dict:
        """snarkjs proof.json as a dict (snarkjs.proof_to_json; write_proof_json writes the file)"""
        from . import snarkjs
        return snarkjs.proof_to_json(self, device, lib)

    @staticmethod
    def from_json(src, device=0, lib: Optional[B.Library] = None) -> "Proof":
        """a proof.json (dict, JSON text or path); every point goes through the codec's validation"""
        from . import snarkjs
        return snarkjs.proof_from_json(src, device, lib)

    def to_eth(self, device=0, lib: Optional[B.Library] = None):
        """ethereum::Proof::as_tuple (reference src/ethereum.rs:104-118): (a, b, c) as ints, G2 with c1 first"""
        from . import snarkjs
        return snarkjs.proof_to_eth(self, device, lib)

    @staticmethod
    def from_eth(t, device=0, lib: Optional[B.Library] = None) -> "Proof":
        from . import snarkjs
        return snarkjs.proof_from_eth(t, device, lib)

    def rerandomize(self, vk, r1=None, r2=None, device=0, lib: Optional[B.Library] = None) -> "Proof":
        """Groth16::rerandomize_proof of this proof (rerandomize): r1 in [1, r) and r2 in [0, r) as ints, or both
        None: drawn by the library from the OS CSPRNG."""
        if (r1 is None) != (r2 is None):
            raise G16Error(B.G16_ERR_INVALID, "give r1 and r2, or neither")
        return rerandomize(vk, [self], None if r1 is None else [(r1, r2)], device=device, lib=lib)[0]


DEFAULT_TABLES = 0     # g16_options.fixed_tables when Prover(tables=None): 0 = the library decides


class Prover:
    """Device-resident (pk, matrices): the state create_proof_with_reduction_and_matrices borrows
    on every call in the reference, uploaded and precomputed once here (g16_ctx_create)."""

    def __init__(self, pk: Optional[ProvingKey], matrices: ConstraintMatrices, device=0, rank=0,
                 world=1, window_bits=0, planes=0, lib: Optional[B.Library] = None,
                 n_vars: Optional[int] = None, dist_wm=False, reduction: str = "circom",
                 devices: Optional[Sequence[int]] = None, shard: str = "auto",
                 sibling_of: Optional["Prover"] = None, tables: Optional[int] = None):
        """devices=[d0, d1, ...]: ONE ctx sharded over several GPUs inside the library
        (g16_ctx_create_multi); prove() / prove_dev() are then used exactly as on one device.
        shard (world > 1 / devices): "points" = point-range MSM shards, "buckets" = every rank holds
        all points of the witness queries and 1/world of their sorted bucket list (H stays cut by
        point range), "auto" = points.
        sibling_of=prover: a second ctx on the same device that borrows `prover`'s point planes
        (g16_ctx_create_sibling): two threads, two proofs in flight.
        tables (g16_options.fixed_tables): None / 0 = automatic (small single-device keys prove through
        fixed-base tables), 1 = require, -1 = never; DEFAULT_TABLES overrides None (the test-suite pins
        the bucket path that way)."""
        self.lib = lib or B.load()
        self.matrices = matrices
        self.pk = pk
        if pk is None:  # witness-map-only context (R1CSToQAP use)
            if n_vars is None:
                # the two producers of ConstraintMatrices disagree on num_witness_variables
                # (read_zkey: n_vars - n_public, src/zkey.rs:183; R1CS: n_wires - num_inputs), so the
                # witness length cannot be derived from the counts: it is max wire index + 1 at least
                raise G16Error(B.G16_ERR_INVALID, "a witness-map-only Prover needs n_vars (len(full_assignment))")
            need = matrices.num_constraints + matrices.num_instance_variables
            dom = 1
            while dom < need:
                dom <<= 1
            kd = B.KeyDesc()
            kd.n_vars, kd.n_public, kd.domain_size = n_vars, matrices.num_instance_variables - 1, dom
        else:
            kd = pk.to_c()
        self.n_vars = kd.n_vars
        self.domain_size = kd.domain_size
        opt = B.Options()
        opt.device, opt.rank, opt.world = device, rank, world
        opt.window_bits, opt.planes = window_bits, planes
        opt.dist_wm = 1 if dist_wm else 0
        opt.reduction = REDUCTIONS[reduction]
        opt.shard = SHARD_MODES[shard]
        opt.fixed_tables = DEFAULT_TABLES if tables is None else int(tables)
        self.dist_wm = bool(opt.dist_wm)
        self.rank, self.world = rank, world
        a, b = matrices.a.to_c(), matrices.b.to_c()
        ctx = C.c_void_p()
        self.devices = list(devices) if devices is not None else None
        self._donor = sibling_of                          # keeps the lender alive
        if sibling_of is not None:
            st = self.lib.g16_ctx_create_sibling(sibling_of.ctx, C.byref(kd), C.byref(a), C.byref(b),
                                                 matrices.num_constraints, C.byref(opt), C.byref(ctx))
        elif self.devices is not None:
            opt.dist_wm = -1 if dist_wm is None else 0   # None: force a replicated witness map
            ids = (C.c_int * len(self.devices))(*self.devices)
            st = self.lib.g16_ctx_create_multi(C.byref(kd), C.byref(a), C.byref(b), matrices.num_constraints,
                                               ids, len(self.devices), C.byref(opt), C.byref(ctx))
        else:
            st = self.lib.g16_ctx_create(C.byref(kd), C.byref(a), C.byref(b), matrices.num_constraints,
                                         C.byref(opt), C.byref(ctx))
        self.lib.check(st, None)
        self.ctx = ctx

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.g16_ctx_destroy(self.ctx)
            self.ctx = None

    __del__ = close

    # -- CircomReduction::witness_map_from_matrices
    def witness_map(self, full_assignment) -> np.ndarray:
        w = _as_fr(full_assignment, self.lib)
        h = np.empty((self.domain_size, 4), dtype=np.uint64)
        self.lib.check(self.lib.g16_witness_map(self.ctx, _np_ptr(w), w.shape[0], _np_ptr(h)), self.ctx)
        return h

    def msm_g1(self, which: int, scalars) -> bytes:
        s = _as_fr(scalars, self.lib)
        out = np.empty(64, dtype=np.uint8)
        self.lib.check(self.lib.g16_msm_g1(self.ctx, which, _np_ptr(s), s.shape[0], _np_ptr(out)), self.ctx)
        return out.tobytes()

    def msm_g2(self, scalars) -> bytes:
        s = _as_fr(scalars, self.lib)
        out = np.empty(128, dtype=np.uint8)
        self.lib.check(self.lib.g16_msm_g2(self.ctx, _np_ptr(s), s.shape[0], _np_ptr(out)), self.ctx)
        return out.tobytes()

    def witness_map_dev(self, w_dev_ptr: int, h_dev_ptr: int):
        self.lib.check(self.lib.g16_witness_map_dev(self.ctx, C.c_void_p(w_dev_ptr), self.n_vars,
                                                    C.c_void_p(h_dev_ptr)), self.ctx)

    def msm_g1_dev(self, which: int, scalars_dev_ptr: int, count: int) -> bytes:
        out = np.empty(64, dtype=np.uint8)
        self.lib.check(self.lib.g16_msm_g1_dev(self.ctx, which, C.c_void_p(scalars_dev_ptr), count,
                                               _np_ptr(out)), self.ctx)
        return out.tobytes()

    def msm_g2_dev(self, scalars_dev_ptr: int, count: int) -> bytes:
        out = np.empty(128, dtype=np.uint8)
        self.lib.check(self.lib.g16_msm_g2_dev(self.ctx, C.c_void_p(scalars_dev_ptr), count,
                                               _np_ptr(out)), self.ctx)
        return out.tobytes()

    def prove(self, r, s, full_assignment) -> Proof:
        w = _as_fr(full_assignment, self.lib)
        rs = _as_fr([r, s], self.lib) if not isinstance(r, np.ndarray) else np.stack([r, s])
        out = np.empty(B.G16_PROOF_BYTES, dtype=np.uint8)
        self.lib.check(self.lib.g16_prove(self.ctx, _np_ptr(rs[0:1]), _np_ptr(rs[1:2]), _np_ptr(w),
                                          w.shape[0], _np_ptr(out)), self.ctx)
        return Proof(out.tobytes())

    def prove_dev(self, r, s, w_dev_ptr: int) -> Proof:
        """witness already resident in HBM (device pointer to n_vars x 32 bytes)"""
        rs = _as_fr([r, s], self.lib) if not isinstance(r, np.ndarray) else np.stack([r, s])
        out = np.empty(B.G16_PROOF_BYTES, dtype=np.uint8)
        self.lib.check(self.lib.g16_prove_dev(self.ctx, _np_ptr(rs[0:1]), _np_ptr(rs[1:2]),
                                              C.c_void_p(w_dev_ptr), self.n_vars, _np_ptr(out)), self.ctx)
        return Proof(out.tobytes())

    def _batch_rs(self, rs):
        rs = list(rs)
        if not rs:
            return np.zeros((0, 4), dtype=np.uint64), np.zeros((0, 4), dtype=np.uint64)
        if all(isinstance(v, np.ndarray) for pair in rs for v in pair):
            r = np.ascontiguousarray(np.stack([np.asarray(p[0], dtype=np.uint64).reshape(4) for p in rs]))
            s = np.ascontiguousarray(np.stack([np.asarray(p[1], dtype=np.uint64).reshape(4) for p in rs]))
            return r, s
        both = _as_fr([v for pair in rs for v in pair], self.lib).reshape(len(rs), 2, 4)
        return np.ascontiguousarray(both[:, 0]), np.ascontiguousarray(both[:, 1])

    def _batch_witnesses(self, witnesses) -> np.ndarray:
        if isinstance(witnesses, np.ndarray) and witnesses.dtype == np.uint64:
            w = np.ascontiguousarray(witnesses)
            if w.ndim != 3 or w.shape[2] != 4:
                raise G16Error(B.G16_ERR_INVALID, "witnesses: a (count, n_vars, 4) uint64 array")
            return w
        ws = [_as_fr(x, self.lib) for x in witnesses]
        if not ws:
            return np.zeros((0, self.n_vars, 4), dtype=np.uint64)
        if any(x.shape != ws[0].shape for x in ws):
            raise G16Error(B.G16_ERR_INVALID, "witnesses: assignments of different lengths")
        return np.ascontiguousarray(np.stack(ws))

    def prove_batch(self, rs, witnesses) -> List[Proof]:
        """proofs of many witnesses under this key (g16_prove_batch): rs = sequence of (r, s), witnesses =
        sequence of full assignments or a (count, n_vars, 4) uint64 Montgomery array.  Proof i equals
        prove(*rs[i], witnesses[i]) byte for byte."""
        r, s = self._batch_rs(rs)
        w = self._batch_witnesses(witnesses)
        if w.shape[0] != r.shape[0]:
            raise G16Error(B.G16_ERR_INVALID, f"{r.shape[0]} (r, s) pairs for {w.shape[0]} witnesses")
        count = r.shape[0]
        out = np.empty(max(count, 1) * B.G16_PROOF_BYTES, dtype=np.uint8)
        self.lib.check(self.lib.g16_prove_batch(self.ctx, count, _np_ptr(r), _np_ptr(s), _np_ptr(w), w.shape[1],
                                                _np_ptr(out)), self.ctx)
        raw = out.tobytes()
        return [Proof(raw[i * B.G16_PROOF_BYTES:(i + 1) * B.G16_PROOF_BYTES]) for i in range(count)]

    def prove_batch_dev(self, rs, w_dev_ptr: int, count: int) -> List[Proof]:
        """witnesses already resident in HBM: device pointer to count x n_vars x 32 bytes, contiguous"""
        r, s = self._batch_rs(rs)
        if r.shape[0] != count:
            raise G16Error(B.G16_ERR_INVALID, f"{r.shape[0]} (r, s) pairs for {count} witnesses")
        if count == 0:
            return []
        out = np.empty(count * B.G16_PROOF_BYTES, dtype=np.uint8)
        self.lib.check(self.lib.g16_prove_batch_dev(self.ctx, count, _np_ptr(r), _np_ptr(s), C.c_void_p(w_dev_ptr),
                                                    self.n_vars, _np_ptr(out)), self.ctx)
        raw = out.tobytes()
        return [Proof(raw[i * B.G16_PROOF_BYTES:(i + 1) * B.G16_PROOF_BYTES]) for i in range(count)]

    def witness_map_batch(self, witnesses) -> np.ndarray:
        """witness_map for many assignments in one pass: (count, domain_size, 4) uint64 Montgomery"""
        w = self._batch_witnesses(witnesses)
        h = np.empty((w.shape[0], self.domain_size, 4), dtype=np.uint64)
        if w.shape[0]:
            self.lib.check(self.lib.g16_witness_map_batch(self.ctx, w.shape[0], _np_ptr(w), w.shape[1], _np_ptr(h)),
                           self.ctx)
        return h

    def prove_partial(self, r, s, full_assignment=None, w_dev_ptr: Optional[int] = None) -> bytes:
        """this rank's G16_PARTIAL_BYTES record: its A, B1, B2, L, H sums and s*A, r*B1"""
        rs = _as_fr([r, s], self.lib) if not isinstance(r, np.ndarray) else np.stack([r, s])
        out = np.empty(B.G16_PARTIAL_BYTES, dtype=np.uint8)
        if w_dev_ptr is not None:
            st = self.lib.g16_prove_partial_dev(self.ctx, _np_ptr(rs[0:1]), _np_ptr(rs[1:2]),
                                                C.c_void_p(w_dev_ptr), self.n_vars, _np_ptr(out))
        else:
            w = _as_fr(full_assignment, self.lib)
            st = self.lib.g16_prove_partial(self.ctx, _np_ptr(rs[0:1]), _np_ptr(rs[1:2]), _np_ptr(w),
                                            w.shape[0], _np_ptr(out))
        self.lib.check(st, self.ctx)
        return out.tobytes()

    # -- fully sharded prover (dist_wm=True): three phases around two all-to-all exchanges
    def exchange_bytes(self) -> int:
        return int(self.lib.g16_dist_exchange_bytes(self.ctx))

    def dist_phase1(self, r, s, w_dev_ptr: int, send_ptr: int):
        rs = _as_fr([r, s], self.lib) if not isinstance(r, np.ndarray) else np.stack([r, s])
        self.lib.check(self.lib.g16_prove_dist_phase1(self.ctx, _np_ptr(rs[0:1]), _np_ptr(rs[1:2]),
                                                      C.c_void_p(w_dev_ptr), self.n_vars,
                                                      C.c_void_p(send_ptr)), self.ctx)

    def dist_phase2(self, recv_ptr: int, send_ptr: int):
        self.lib.check(self.lib.g16_prove_dist_phase2(self.ctx, C.c_void_p(recv_ptr),
                                                      C.c_void_p(send_ptr)), self.ctx)

    def dist_phase3(self, recv_ptr: int) -> bytes:
        out = np.empty(B.G16_PARTIAL_BYTES, dtype=np.uint8)
        self.lib.check(self.lib.g16_prove_dist_phase3(self.ctx, C.c_void_p(recv_ptr), _np_ptr(out)),
                       self.ctx)
        return out.tobytes()

    def prove_finish(self, r, s, partials: bytes) -> Proof:
        rs = _as_fr([r, s], self.lib) if not isinstance(r, np.ndarray) else np.stack([r, s])
        world = len(partials) // B.G16_PARTIAL_BYTES
        buf = np.frombuffer(partials, dtype=np.uint8)
        out = np.empty(B.G16_PROOF_BYTES, dtype=np.uint8)
        self.lib.check(self.lib.g16_prove_finish(self.ctx, _np_ptr(rs[0:1]), _np_ptr(rs[1:2]),
                                                 _np_ptr(buf), world, _np_ptr(out)), self.ctx)
        return Proof(out.tobytes())

    def witness_buffer(self) -> int:
        return int(self.lib.g16_witness_buffer(self.ctx) or 0)

    def upload_witness(self, full_assignment) -> int:
        """witness resident in HBM (on every device of a multi-device ctx); returns the pointer to
        pass to prove_dev()"""
        w = _as_fr(full_assignment, self.lib)
        self.lib.check(self.lib.g16_witness_upload(self.ctx, _np_ptr(w), w.shape[0]), self.ctx)
        return self.witness_buffer()

    # -- canonical witnesses: a .wtns goes to the device as it lies in the file (g16_*_canonical)
    def _canonical_witness(self, wtns):
        """((n_vars, 32) uint8 canonical values, keepalive) of a path, bytes, a Witness or such an array"""
        if isinstance(wtns, np.ndarray):
            return _canonical_bytes(wtns), None
        w = wtns if isinstance(wtns, Witness) else open_wtns(wtns, self.lib)
        return w.canonical, w

    @staticmethod
    def _draw_rs(r, s):
        rng = random.SystemRandom()   # as Groth16.prove draws them
        return (rng.randrange(FR_MODULUS) if r is None else r), (rng.randrange(FR_MODULUS) if s is None else s)

    def prove_wtns(self, wtns, r=None, s=None) -> Proof:
        """prove(r, s, read_wtns(wtns)) byte for byte, without the host conversion (g16_prove_canonical): wtns = path,
        bytes, Witness or a (n_vars, 32) uint8 array of canonical values.  r, s: ints or Montgomery limbs; None =
        drawn as Groth16.prove draws them.  A value >= r raises G16Error naming the element."""
        w, _keep = self._canonical_witness(wtns)
        r, s = self._draw_rs(r, s)
        rs = _as_fr([r, s], self.lib) if not isinstance(r, np.ndarray) else np.stack([r, s])
        out = np.empty(B.G16_PROOF_BYTES, dtype=np.uint8)
        self.lib.check(self.lib.g16_prove_canonical(self.ctx, _np_ptr(rs[0:1]), _np_ptr(rs[1:2]), _np_ptr(w),
                                                    w.shape[0], _np_ptr(out)), self.ctx)
        return Proof(out.tobytes())

    def prove_wtns_batch(self, wtns_list, rs=None) -> List[Proof]:
        """prove_batch for canonical witnesses (g16_prove_batch_canonical): one conversion launch per chunk ahead of
        the batched prover.  rs: sequence of (r, s), None = drawn.  A value >= r raises G16Error naming the proof and
        the element, with first_bad = proof * n_vars + element; no proof is returned."""
        ws = [self._canonical_witness(x) for x in wtns_list]
        count = len(ws)
        if rs is None:
            rs = [self._draw_rs(None, None) for _ in range(count)]
        r, s = self._batch_rs(rs)
        if r.shape[0] != count:
            raise G16Error(B.G16_ERR_INVALID, f"{r.shape[0]} (r, s) pairs for {count} witnesses")
        if count == 0:
            return []
        if any(w.shape[0] != self.n_vars for w, _ in ws):
            raise G16Error(B.G16_ERR_INVALID, "witness length != n_vars of the key")
        w = np.ascontiguousarray(np.stack([x for x, _ in ws]))
        out = np.empty(count * B.G16_PROOF_BYTES, dtype=np.uint8)
        bad = C.c_int64(-1)
        st = self.lib.g16_prove_batch_canonical(self.ctx, count, _np_ptr(r), _np_ptr(s), _np_ptr(w), self.n_vars,
                                                _np_ptr(out), C.byref(bad))
        _check_canonical(self.lib, st, self.ctx, bad)
        raw = out.tobytes()
        return [Proof(raw[i * B.G16_PROOF_BYTES:(i + 1) * B.G16_PROOF_BYTES]) for i in range(count)]

    def upload_witness_canonical(self, wtns) -> int:
        """upload_witness for canonical values (g16_witness_upload_canonical); returns the pointer for prove_dev()"""
        w, _keep = self._canonical_witness(wtns)
        bad = C.c_int64(-1)
        st = self.lib.g16_witness_upload_canonical(self.ctx, _np_ptr(w), w.shape[0], C.byref(bad))
        _check_canonical(self.lib, st, self.ctx, bad)
        return self.witness_buffer()

    def witness_host_buffer(self) -> np.ndarray:
        """(n_vars, 4) uint64 view of the ctx's page-locked staging buffer (g16_witness_host_buffer)"""
        p = self.lib.g16_witness_host_buffer(self.ctx)
        if not p:
            raise G16Error(B.G16_ERR_HIP, "pinned allocation failed")
        arr = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint64)), shape=(self.n_vars * 4,))
        return arr.reshape(self.n_vars, 4)

    # -- device-side hand-offs for a host framework that owns a stream (torch + RCCL)
    def set_exchange_stream(self, hip_stream: int, enabled=True):
        self.lib.check(self.lib.g16_dist_set_exchange_stream(self.ctx, C.c_void_p(hip_stream),
                                                             1 if enabled else 0), self.ctx)

    def partial_buffer(self) -> int:
        return int(self.lib.g16_partial_buffer(self.ctx) or 0)

    def gather_buffer(self) -> int:
        return int(self.lib.g16_gather_buffer(self.ctx) or 0)

    def dist_phase3_dev(self, recv_ptr: int):
        """phase 3 with the record left in partial_buffer() (needs set_exchange_stream)"""
        self.lib.check(self.lib.g16_prove_dist_phase3(self.ctx, C.c_void_p(recv_ptr), None), self.ctx)

    def prove_finish_dev(self, r, s) -> Proof:
        rs = _as_fr([r, s], self.lib) if not isinstance(r, np.ndarray) else np.stack([r, s])
        out = np.empty(B.G16_PROOF_BYTES, dtype=np.uint8)
        self.lib.check(self.lib.g16_prove_finish_dev(self.ctx, _np_ptr(rs[0:1]), _np_ptr(rs[1:2]),
                                                     _np_ptr(out)), self.ctx)
        return Proof(out.tobytes())

    def attach_rccl(self, nccl_comm: int):
        """hand the library an ncclComm_t the host created over the same ranks (g16_dist_attach_rccl): the
        collectives of prove_dist() are then issued by the library itself"""
        self.lib.check(self.lib.g16_dist_attach_rccl(self.ctx, C.c_void_p(nccl_comm)), self.ctx)

    def rccl_ranks(self) -> int:
        return int(self.lib.g16_dist_rccl_ranks(self.ctx))

    def prove_dist(self, r, s, w_dev_ptr: int) -> Proof:
        """one whole sharded proof of this rank through the attached communicator (g16_prove_dist)"""
        rs = _as_fr([r, s], self.lib) if not isinstance(r, np.ndarray) else np.stack([r, s])
        out = np.empty(B.G16_PROOF_BYTES, dtype=np.uint8)
        self.lib.check(self.lib.g16_prove_dist(self.ctx, _np_ptr(rs[0:1]), _np_ptr(rs[1:2]), C.c_void_p(w_dev_ptr),
                                               self.n_vars, _np_ptr(out)), self.ctx)
        return Proof(out.tobytes())

    def set_profiling(self, on: bool):
        self.lib.check(self.lib.g16_set_profiling(self.ctx, 1 if on else 0), self.ctx)

    def stage_times(self):
        ms = (C.c_float * B.G16_N_STAGES)()
        cnt = (C.c_uint32 * B.G16_N_STAGES)()
        self.lib.check(self.lib.g16_stage_times(self.ctx, ms, cnt), self.ctx)
        return {self.lib.g16_stage_name(i).decode(): (float(ms[i]), int(cnt[i]))
                for i in range(B.G16_N_STAGES)}

    def links(self):
        """multi-device ctx: the create-time link probe (g16_multi_links) as
        {"probe_bytes", "gbps": [[src][dst]], "echo_us": [[src][dst]]}"""
        n = self.info()["devices"]
        gb, us = (C.c_float * (n * n))(), (C.c_float * (n * n))()
        pb = C.c_uint64(0)
        self.lib.check(self.lib.g16_multi_links(self.ctx, gb, us, n * n, C.byref(pb)), self.ctx)
        return {"probe_bytes": int(pb.value), "gbps": [[float(gb[a * n + b]) for b in range(n)] for a in range(n)],
                "echo_us": [[float(us[a * n + b]) for b in range(n)] for a in range(n)]}

    def info(self):
        out = (C.c_uint32 * 16)()
        self.lib.check(self.lib.g16_ctx_info(self.ctx, out), self.ctx)
        keys = ["c_w", "W_w", "planes_w", "D_w", "c_h", "W_h", "planes_h", "D_h", "domain_size",
                "log_n", "shard_w", "shard_h", "devices", "shard_mode", "peer_access", "fixed_tables"]
        d = dict(zip(keys, list(out)))
        d["shard_mode"] = {0: "none", 1: "points", 2: "buckets"}.get(d["shard_mode"], "?")
        d["sparse_b"] = (d["fixed_tables"] >> 1) & 1       # out[15]: bit 0 = fixed-base tables, bit 1 = filtered B view
        d["batched"] = (d["fixed_tables"] >> 2) & 1        # bit 2 = a chunk of prove_batch is enqueued once
        d["fixed_tables"] &= 1
        return d


def _transpose_csr(m: Csr, n_cols: int, extra=None) -> Csr:
    """CSR (rows = constraints) -> CSR of the transpose (rows = wires).  extra: optional
    (rows, cols, coeff) triplets appended before transposing."""
    counts = np.diff(m.row_ptr.astype(np.int64))
    rows = np.repeat(np.arange(m.num_rows, dtype=np.int64), counts)
    cols = m.col.astype(np.int64)
    vals = m.coeff
    if extra is not None:
        rows = np.concatenate([rows, np.asarray(extra[0], dtype=np.int64)])
        cols = np.concatenate([cols, np.asarray(extra[1], dtype=np.int64)])
        vals = np.concatenate([vals, np.asarray(extra[2], dtype=np.uint64).reshape(-1, 4)])
    order = np.argsort(cols, kind="stable")
    rp = np.zeros(n_cols + 1, dtype=np.int64)
    np.cumsum(np.bincount(cols, minlength=n_cols), out=rp[1:])
    return Csr(rp.astype(np.uint32), rows[order].astype(np.uint32), vals[order])


REDUCTIONS = {"circom": 0, "libsnark": 1}
SHARD_MODES = {"auto": B.SHARD_AUTO, "points": B.SHARD_POINTS, "buckets": B.SHARD_BUCKETS}


def _setup_matrices(a: Csr, b: Csr, c: Csr, n_vars: int, n_public: int, lib):
    """the transposed matrices g16_setup_create_ex / g16_setup_from_srs take: rows = wires, `at` with the
    n_public + 1 rows snarkjs appends"""
    m = a.num_rows
    ni = n_public + 1
    one = fr_from_ints([1], lib)
    at = _transpose_csr(a, n_vars, (np.arange(m, m + ni), np.arange(ni), np.tile(one, (ni, 1))))
    return at, _transpose_csr(b, n_vars), _transpose_csr(c, n_vars)


def _setup_key(lib, h, n_vars: int, n_public: int) -> ProvingKey:
    """ProvingKey over the host arrays a g16_setup handle owns"""
    handle = _Handle(lib, h, lib.g16_setup_destroy)
    kd = B.KeyDesc()
    icp = C.c_void_p()
    cnt = C.c_uint32()
    gamma = (C.c_uint8 * 128)()
    lib.check(lib.g16_setup_key(h, C.byref(kd), C.byref(icp), C.byref(cnt), gamma))

    vk = VerifyingKey(bytes(kd.alpha_g1), bytes(kd.beta_g2), bytes(gamma), bytes(kd.delta_g2),
                      _view(icp, cnt.value, 64).copy())
    return ProvingKey(kd.n_vars, kd.n_public, kd.domain_size, vk, bytes(kd.beta_g1), bytes(kd.delta_g1),
                      _view(kd.a_query, n_vars, 64), _view(kd.b_g1_query, n_vars, 64),
                      _view(kd.b_g2_query, n_vars, 128), _view(kd.l_query, n_vars - n_public - 1, 64),
                      _view(kd.h_query, kd.domain_size, 64), keepalive=handle)


def trapdoor_setup(a: Csr, b: Csr, c: Csr, n_vars: int, n_public: int, toxic: Sequence[int],
                   device=0, lib: Optional[B.Library] = None, reduction: str = "circom") -> ProvingKey:
    """Known-toxic-waste setup on the GPU (g16_setup_create_ex): the key
    Groth16::generate_random_parameters_with_reduction::<QAP> would produce for
    (tau, alpha, beta, gamma, delta) = toxic, QAP = CircomReduction ("circom", snarkjs-compatible)
    or LibsnarkReduction ("libsnark", arkworks' default: reference tests/groth16.rs:25).
    Used to mint the synthetic BASELINE keys."""
    lib = lib or B.load()
    at, bt, ct = _setup_matrices(a, b, c, n_vars, n_public, lib)
    tox = fr_from_ints(list(toxic), lib)
    h = C.c_void_p()
    cat, cbt, cct = at.to_c(), bt.to_c(), ct.to_c()
    st = lib.g16_setup_create_ex(device, C.byref(cat), C.byref(cbt), C.byref(cct), n_vars, n_public, a.num_rows,
                                 _np_ptr(tox), REDUCTIONS[reduction], C.byref(h))
    if st != B.G16_OK:
        raise (SynthesisError if st == B.G16_ERR_DOMAIN_TOO_LARGE else G16Error)(st, "g16_setup_create failed")
    return _setup_key(lib, h, n_vars, n_public)


class Srs:
    """A powers-of-tau string as g16_setup_from_srs reads it (sections 2-6 of a snarkjs .ptau): packed affine
    points in the zkey encoding, one per row.  tau_g1: (>= 2 domain - 1, 64) uint8, tau^i G1; tau_g2:
    (>= domain, 128), tau^i G2; alpha_tau_g1 / beta_tau_g1: (>= domain, 64), alpha tau^i G1 / beta tau^i G1;
    beta_g2: 128 bytes.  Arrays a caller supplies are taken as they are: check_srs tells whether they are a
    consistent powers-of-tau string.  power / ceremony_power: the header of the .ptau it was read from, else None."""
    power = ceremony_power = None

    def __init__(self, tau_g1, tau_g2, alpha_tau_g1, beta_tau_g1, beta_g2, keepalive=None):
        self.tau_g1 = np.ascontiguousarray(tau_g1, dtype=np.uint8).reshape(-1, 64)
        self.tau_g2 = np.ascontiguousarray(tau_g2, dtype=np.uint8).reshape(-1, 128)
        self.alpha_tau_g1 = np.ascontiguousarray(alpha_tau_g1, dtype=np.uint8).reshape(-1, 64)
        self.beta_tau_g1 = np.ascontiguousarray(beta_tau_g1, dtype=np.uint8).reshape(-1, 64)
        self.beta_g2 = bytes(beta_g2)
        if len(self.beta_g2) != 128:
            raise G16Error(B.G16_ERR_INVALID, "beta_g2 is one packed G2 point: 128 bytes")
        self._keepalive = keepalive

    def to_c(self) -> B.SrsDesc:
        d = B.SrsDesc()
        d.n_tau_g1 = self.tau_g1.shape[0]
        d.n_tau = min(self.tau_g2.shape[0], self.alpha_tau_g1.shape[0], self.beta_tau_g1.shape[0])
        d.tau_g1, d.tau_g2 = self.tau_g1.ctypes.data, self.tau_g2.ctypes.data
        d.alpha_tau_g1, d.beta_tau_g1 = self.alpha_tau_g1.ctypes.data, self.beta_tau_g1.ctypes.data
        C.memmove(d.beta_g2, self.beta_g2, 128)
        return d


def trapdoor_srs(log2_domain: int, toxic: Sequence[int], device=0, lib: Optional[B.Library] = None) -> Srs:
    """An SRS for domains up to 2^log2_domain from a trapdoor the caller knows, toxic = (tau, alpha, beta), on
    the GPU (g16_srs_create) -- for tests and synthetic keys; a real ceremony's string comes from its .ptau."""
    lib = lib or B.load()
    if len(toxic) != 3:
        raise G16Error(B.G16_ERR_INVALID, "toxic = (tau, alpha, beta)")
    tox = fr_from_ints(list(toxic), lib)
    h = C.c_void_p()
    st = lib.g16_srs_create(device, int(log2_domain), _np_ptr(tox), C.byref(h))
    if st != B.G16_OK:
        raise (SynthesisError if st == B.G16_ERR_DOMAIN_TOO_LARGE else G16Error)(st, "g16_srs_create failed")
    handle = _Handle(lib, h, lib.g16_srs_destroy)
    d = B.SrsDesc()
    lib.check(lib.g16_srs_desc_of(h, C.byref(d)))

    return Srs(_view(d.tau_g1, d.n_tau_g1, 64), _view(d.tau_g2, d.n_tau, 128), _view(d.alpha_tau_g1, d.n_tau, 64),
               _view(d.beta_tau_g1, d.n_tau, 64), bytes(d.beta_g2), keepalive=handle)


class LagrangeSrs:
    """The Lagrange sections 12-15 of a prepared .ptau (`snarkjs powersoftau prepare phase2`), the layout of
    include/g16_amd.h: tau_g1 (2^(power+2) - 1, 64) uint8 in levels 0 .. power + 1; tau_g2 (2^(power+1) - 1, 128),
    alpha_tau_g1 and beta_tau_g1 (2^(power+1) - 1, 64) in levels 0 .. power.  Level p starts at row 2^p - 1 and holds
    the 2^p points L_j(tau) G of the domain of size 2^p.  Arrays a caller supplies are taken as they are:
    check_lagrange tells whether they belong to an Srs."""
    ARRAYS = B.LAGRANGE_ARRAYS

    def __init__(self, power, tau_g1, tau_g2, alpha_tau_g1, beta_tau_g1, keepalive=None):
        self.power = int(power)
        if not 0 <= self.power <= 27:
            raise SynthesisError(B.G16_ERR_DOMAIN_TOO_LARGE, "a Lagrange set has power <= 27")
        self.tau_g1 = np.ascontiguousarray(tau_g1, dtype=np.uint8).reshape(-1, 64)
        self.tau_g2 = np.ascontiguousarray(tau_g2, dtype=np.uint8).reshape(-1, 128)
        self.alpha_tau_g1 = np.ascontiguousarray(alpha_tau_g1, dtype=np.uint8).reshape(-1, 64)
        self.beta_tau_g1 = np.ascontiguousarray(beta_tau_g1, dtype=np.uint8).reshape(-1, 64)
        m1, m2 = (4 << self.power) - 1, (2 << self.power) - 1
        if (self.tau_g1.shape[0], self.tau_g2.shape[0], self.alpha_tau_g1.shape[0],
                self.beta_tau_g1.shape[0]) != (m1, m2, m2, m2):
            raise G16Error(B.G16_ERR_INVALID, f"a Lagrange set of power {self.power} has {m1} tau_g1 points and "
                                              f"{m2} of each other array")
        self._keepalive = keepalive

    def levels(self, name) -> int:
        """levels of the array: power + 2 for tau_g1, power + 1 for the others"""
        if name not in self.ARRAYS:
            raise G16Error(B.G16_ERR_INVALID, f"no array {name!r}")
        return self.power + (2 if name == "tau_g1" else 1)

    def level(self, name, p):
        """view of level p of the array: 2^p rows"""
        p = int(p)
        if not 0 <= p < self.levels(name):
            raise G16Error(B.G16_ERR_INVALID, f"{name} has no level {p}")
        return getattr(self, name)[(1 << p) - 1:(2 << p) - 1]

    @staticmethod
    def locate(index):
        """position in a section -> (level, j)"""
        p = (int(index) + 1).bit_length() - 1
        return p, int(index) + 1 - (1 << p)

    def to_c(self) -> B.SrsLagrangeDesc:
        d = B.SrsLagrangeDesc()
        d.power = self.power
        d.tau_g1, d.tau_g2 = self.tau_g1.ctypes.data, self.tau_g2.ctypes.data
        d.alpha_tau_g1, d.beta_tau_g1 = self.alpha_tau_g1.ctypes.data, self.beta_tau_g1.ctypes.data
        return d


def _srs_power(d: B.SrsDesc) -> int:
    """the largest power of a .ptau the arrays cover (write_ptau's rule)"""
    power = 0
    while power < 28 and d.n_tau >= 2 << power and d.n_tau_g1 >= (4 << power) - 1:
        power += 1
    return power


def prepare_phase2(srs: Srs, power=None, device=0, lib: Optional[B.Library] = None) -> LagrangeSrs:
    """`snarkjs powersoftau prepare phase2` on the GPU (g16_srs_prepare): every level of the Lagrange copies of
    the four arrays, by the group transform of setup_from_srs.  power: None = the largest the arrays cover (at most
    27); entries of srs beyond 2^(power+1) - 1 / 2^power are dropped.  The same bytes on every run."""
    lib = lib or B.load()
    d = srs.to_c()
    power = min(_srs_power(d), 27) if power is None else int(power)
    if power < 0:
        raise G16Error(B.G16_ERR_INVALID, "power >= 0")
    if power > 27:
        raise SynthesisError(B.G16_ERR_DOMAIN_TOO_LARGE, "g16_srs_prepare: power > 27")
    if d.n_tau < 1 << power or d.n_tau_g1 < (2 << power) - 1:
        raise G16Error(B.G16_ERR_INVALID, "the SRS is shorter than 2^power")
    m1, m2 = (4 << power) - 1, (2 << power) - 1
    tau_g1 = np.empty((m1, 64), dtype=np.uint8)
    tau_g2 = np.empty((m2, 128), dtype=np.uint8)
    alpha = np.empty((m2, 64), dtype=np.uint8)
    beta = np.empty((m2, 64), dtype=np.uint8)
    st = lib.g16_srs_prepare(device, C.byref(d), power, _np_ptr(tau_g1), _np_ptr(tau_g2), _np_ptr(alpha),
                             _np_ptr(beta))
    if st != B.G16_OK:
        raise (SynthesisError if st == B.G16_ERR_DOMAIN_TOO_LARGE else G16Error)(st, "g16_srs_prepare failed")
    return LagrangeSrs(power, tau_g1, tau_g2, alpha, beta)


def prepare_phase2_times(lib: Optional[B.Library] = None) -> dict:
    """milliseconds per phase of this thread's last prepare_phase2 (g16_srs_prepare_times), the phases of
    setup_from_srs_times"""
    return _phase_times(lib, "g16_srs_prepare_times", SETUP_SRS_PHASES)


class _CheckReport:
    """What the reports of check_key, check_contribution, check_srs and check_lagrange share: the verdict fields,
    the per-query count dicts, equality (same class, same fields) and the skeleton of describe().  A report class
    gives its RELATIONS (bit, words), the attribute that holds its bad-point list (LIST; an entry ends with its
    reason bits) and how it names an entry (_where)."""
    REASONS = ((B.KEY_BAD_NONCANONICAL, "non-canonical coordinate"), (B.KEY_BAD_OFF_CURVE, "off the curve"),
               (B.KEY_BAD_SUBGROUP, "outside the prime-order subgroup"))
    RELATIONS = ()
    SINGLES = ()
    LIST = "bad"

    def _fill(self, rep, names=()):
        self.ok = bool(rep.ok)
        self.relations_checked = bool(rep.relations_checked)
        self.relations_failed = int(rep.relations_failed)
        if names:
            self.n_points = {q: int(rep.n_points[i]) for i, q in enumerate(names)}
            self.n_bad = {q: int(rep.n_bad[i]) for i, q in enumerate(names)}
            self.n_infinity = {q: int(rep.n_infinity[i]) for i, q in enumerate(names)}

    def __eq__(self, o):
        return isinstance(o, type(self)) and vars(o) == vars(self)

    def __repr__(self):
        return f"{type(self).__name__}({self.describe()})"

    def _where(self, entry):
        q, i = entry[0], entry[1]
        return f"{self.SINGLES[i]}" if q == "singles" else f"{q}[{i}]"

    def _bad_words(self):
        return f"{sum(self.n_bad.values())} bad point(s) in all"

    def _relation_words(self):
        return "; ".join(w for bit, w in self.RELATIONS if self.relations_failed & bit)

    def _unlisted_words(self):
        if not self.relations_checked:
            return f"{sum(self.n_bad.values())} bad point(s)"
        return self._relation_words()

    def describe(self) -> str:
        if self.ok:
            return "ok"
        bad = getattr(self, self.LIST)
        if bad:
            why = bad[0][-1]
            words = ", ".join(w for bit, w in self.REASONS if why & bit)
            return f"{self._where(bad[0])}: {words} (reason {why}); {self._bad_words()}"
        return self._unlisted_words()


class LagrangeReport(_CheckReport):
    """g16_srs_lagrange_report + the bad-point list of g16_srs_lagrange_check.  ok: no bad point and no failed
    relation; relations_checked: False when a structural failure made the relations meaningless;
    relations_failed: bit (1 << array), failed_arrays the names; n_points / n_bad / n_infinity: dicts by array
    name; bad_points: [(array_name, level, j, reason_bits)] in ascending (array, position) order, at most
    max_listed."""
    LIST = "bad_points"

    def __init__(self, rep: B.SrsLagrangeReportC, bad):
        self._fill(rep, B.LAGRANGE_ARRAYS)
        self.failed_arrays = [q for i, q in enumerate(B.LAGRANGE_ARRAYS) if self.relations_failed >> i & 1]
        self.bad_points = [(B.LAGRANGE_ARRAYS[b.query],) + LagrangeSrs.locate(b.index) + (int(b.reason),)
                           for b in bad]

    def _where(self, entry):
        return f"{entry[0]} level {entry[1]} entry {entry[2]}"

    def _relation_words(self):
        return "; ".join(f"the Lagrange levels of {q} are not the transforms of its powers"
                         for q in self.failed_arrays)


def check_lagrange(srs: Srs, lag: LagrangeSrs, rho=None, device=0, max_listed=64,
                   lib: Optional[B.Library] = None) -> LagrangeReport:
    """Are the Lagrange sections of a prepared .ptau the transforms of THIS string's powers
    (g16_srs_lagrange_check, on the GPU): every Lagrange point canonical, on its curve and (G2) in the subgroup;
    then, per array, one random 128-bit combination over all its levels against one full-width combination over
    the powers.  srs is expected to have passed check_srs.  A wrong entry passes with probability at most 2^-127.
    rho: None (drawn by the library from the OS CSPRNG) or (2^(power+2) - 1) + 3 (2^(power+1) - 1) ints in
    [1, 2^128): tau_g1, tau_g2, alpha_tau_g1, beta_tau_g1 in this order, levels ascending."""
    lib = lib or B.load()
    d, dl = srs.to_c(), lag.to_c()
    rho_arr = _rho_array(rho, ((4 << lag.power) - 1) + 3 * ((2 << lag.power) - 1),
                         "one coefficient per Lagrange point")
    max_listed = int(max_listed)
    bad = (B.KeyBadPoint * max(max_listed, 1))()
    rep = B.SrsLagrangeReportC()
    st = lib.g16_srs_lagrange_check(device, C.byref(d), C.byref(dl), _np_ptr(rho_arr) if rho_arr is not None else None,
                                    bad, max_listed, C.byref(rep))
    if st != B.G16_OK:
        raise (SynthesisError if st == B.G16_ERR_DOMAIN_TOO_LARGE else G16Error)(st, "g16_srs_lagrange_check failed")
    return LagrangeReport(rep, bad[:rep.n_listed])


def setup_from_srs(a: Csr, b: Csr, c: Csr, n_vars: int, n_public: int, srs: Srs, device=0,
                   lib: Optional[B.Library] = None, reduction: str = "circom",
                   lagrange: Optional[LagrangeSrs] = None) -> ProvingKey:
    """The initial key (gamma = delta = 1) of a circuit from a powers-of-tau string, on the GPU
    (g16_setup_from_srs): what `snarkjs zkey new` computes of the points, nobody knowing tau, alpha or beta.
    Matrix arguments and reduction as trapdoor_setup takes them; byte for byte the key trapdoor_setup mints
    for (tau, alpha, beta, 1, 1).  contribute_key then re-randomises delta.  The SRS is NOT verified here:
    check_srs / read_ptau(validate=True) do that.
    lagrange: the string's LagrangeSrs (prepare_phase2, read_ptau(lagrange=True)): no transform is computed, the
    bases are read from it (g16_setup_from_prepared).  The same key when the circuit's domain is 2^power; below
    that every field but the circom h_query is, which is then the one `snarkjs zkey new` writes: it differs from
    the default's point by point and yields the same proofs (include/g16_amd.h).  NOT verified here either:
    check_lagrange does that."""
    lib = lib or B.load()
    at, bt, ct = _setup_matrices(a, b, c, n_vars, n_public, lib)
    h = C.c_void_p()
    cat, cbt, cct = at.to_c(), bt.to_c(), ct.to_c()
    d = srs.to_c()
    if lagrange is not None:
        dl = lagrange.to_c()
        st = lib.g16_setup_from_prepared(device, C.byref(cat), C.byref(cbt), C.byref(cct), n_vars, n_public,
                                         a.num_rows, C.byref(d), C.byref(dl), REDUCTIONS[reduction], C.byref(h))
        what = "g16_setup_from_prepared failed"
    else:
        st = lib.g16_setup_from_srs(device, C.byref(cat), C.byref(cbt), C.byref(cct), n_vars, n_public, a.num_rows,
                                    C.byref(d), REDUCTIONS[reduction], C.byref(h))
        what = "g16_setup_from_srs failed"
    if st != B.G16_OK:
        raise (SynthesisError if st == B.G16_ERR_DOMAIN_TOO_LARGE else G16Error)(st, what)
    return _setup_key(lib, h, n_vars, n_public)


def read_ptau(src, validate=False, lagrange=False, lib: Optional[B.Library] = None) -> Srs:
    """snarkjs .ptau (a path, or bytes) -> Srs, with .power and .ceremony_power (g16_ptau_open; the arrays are
    views of the mapped file).  validate=True runs check_srs (on the GPU) and raises G16Error naming the first
    bad point or the failed relation; the default looks at no point.  The contribution transcript of the file
    is not verified either way.
    lagrange=True: the file must be prepared (sections 12-15, g16_ptau_lagrange); the result has .lagrange, a
    LagrangeSrs of views, and validate=True runs check_lagrange after check_srs.  The default ignores those
    sections, whatever they hold."""
    lib = lib or B.load()
    h = C.c_void_p()
    if isinstance(src, (bytes, bytearray, memoryview)):
        buf = np.frombuffer(bytes(src), dtype=np.uint8)
        lib.check(lib.g16_ptau_open_mem(_np_ptr(buf), buf.shape[0], C.byref(h)), loader=True)
    else:
        lib.check(lib.g16_ptau_open(os.fsencode(src), C.byref(h)), loader=True)
    handle = _Handle(lib, h, lib.g16_ptau_close)
    hdr = B.PtauHeader()
    lib.check(lib.g16_ptau_header_get(h, C.byref(hdr)), loader=True)
    d = B.SrsDesc()
    lib.check(lib.g16_ptau_srs(h, C.byref(d)), loader=True)

    srs = Srs(_view(d.tau_g1, d.n_tau_g1, 64), _view(d.tau_g2, d.n_tau, 128), _view(d.alpha_tau_g1, d.n_tau, 64),
              _view(d.beta_tau_g1, d.n_tau, 64), bytes(d.beta_g2), keepalive=handle)
    srs.power, srs.ceremony_power = int(hdr.power), int(hdr.ceremony_power)
    if lagrange:
        dl = B.SrsLagrangeDesc()
        lib.check(lib.g16_ptau_lagrange(h, C.byref(dl)), loader=True)
        m1, m2 = (4 << dl.power) - 1, (2 << dl.power) - 1
        srs.lagrange = LagrangeSrs(dl.power, _view(dl.tau_g1, m1, 64), _view(dl.tau_g2, m2, 128),
                                   _view(dl.alpha_tau_g1, m2, 64), _view(dl.beta_tau_g1, m2, 64), keepalive=handle)
    if validate:
        rep = check_srs(srs, lib=lib)
        if not rep.ok:
            raise G16Error(B.G16_ERR_INVALID, "ptau failed validation: " + rep.describe())
        if lagrange:
            lrep = check_lagrange(srs, srs.lagrange, lib=lib)
            if not lrep.ok:
                raise G16Error(B.G16_ERR_INVALID, "ptau failed validation: " + lrep.describe())
    return srs


def write_ptau(path, srs: Srs, lagrange: Optional[LagrangeSrs] = None, lib: Optional[B.Library] = None):
    """Srs -> snarkjs .ptau (g16_ptau_write) of the largest power the arrays cover: sections 1-6 and an empty
    contribution list, entries beyond 2^power dropped.  lagrange: a PREPARED file of lagrange.power
    (g16_ptau_write_prepared): sections 12-15 as well."""
    lib = lib or B.load()
    d = srs.to_c()
    if lagrange is not None:
        dl = lagrange.to_c()
        lib.check(lib.g16_ptau_write_prepared(os.fsencode(path), C.byref(d), C.byref(dl), lagrange.power),
                  loader=True)
        return
    lib.check(lib.g16_ptau_write(os.fsencode(path), C.byref(d), _srs_power(d)), loader=True)


class SrsReport(_CheckReport):
    """g16_srs_report + the bad-point list of g16_srs_check.  ok: no bad point and no failed relation;
    relations_checked: False when a structural failure made the pairing relations meaningless;
    relations_failed: SRS_* bits (_binding); n_points / n_bad / n_infinity: dicts by array name
    (_binding.SRS_QUERIES); bad_points: [(array_name, index, reason_bits)] in ascending (array, index) order, at
    most max_listed."""
    RELATIONS = ((B.SRS_BASE, "tau_g1[0] / tau_g2[0] are not the generators"),
                 (B.SRS_DEGENERATE, "tau, alpha or beta is zero"),
                 (B.SRS_PAIR_TAU, "e(tau_g1[1], g2) != e(g1, tau_g2[1])"),
                 (B.SRS_PAIR_TAU_G1, "tau_g1 is not a sequence of powers of tau"),
                 (B.SRS_PAIR_TAU_G2, "tau_g2 is not a sequence of powers of tau"),
                 (B.SRS_PAIR_ALPHA, "alpha_tau_g1 is not a sequence of powers of tau"),
                 (B.SRS_PAIR_BETA, "beta_tau_g1 is not a sequence of powers of tau"),
                 (B.SRS_PAIR_BETA_G2, "e(beta_tau_g1[0], g2) != e(g1, beta_g2)"))
    SINGLES = B.SRS_SINGLES
    LIST = "bad_points"

    def __init__(self, rep: B.SrsReportC, bad):
        self._fill(rep, B.SRS_QUERIES)
        self.bad_points = [(B.SRS_QUERIES[b.query], int(b.index), int(b.reason)) for b in bad]


def check_srs(srs: Srs, rho=None, device=0, max_listed=64, lib: Optional[B.Library] = None) -> SrsReport:
    """Validation of a powers-of-tau string on the GPU (g16_srs_check), the point arithmetic of `snarkjs
    powersoftau verify`: every point canonical, on its curve and (G2) in the prime-order subgroup; then the
    bases are the generators, tau_g1 and tau_g2 hold the same tau, every array is a sequence in that one ratio
    and beta_g2 matches beta_tau_g1[0].  Call it once on an SRS you did not mint, before setup_from_srs or
    check_key_circuit build on it.  The ceremony's contribution transcript is NOT verified: a passing report
    says nothing about who knows tau.
    rho: None (drawn by the library from the OS CSPRNG) or (len(tau_g1) - 1) + 3 (n_tau - 1) ints in
    [1, 2^128), the coefficients of tau_g1, tau_g2, alpha_tau_g1, beta_tau_g1 in this order."""
    lib = lib or B.load()
    d = srs.to_c()
    rho_arr = _rho_array(rho, (d.n_tau_g1 - 1) + 3 * (d.n_tau - 1), "one coefficient per pair of neighbours")
    max_listed = int(max_listed)
    bad = (B.KeyBadPoint * max(max_listed, 1))()
    rep = B.SrsReportC()
    st = lib.g16_srs_check(device, C.byref(d), _np_ptr(rho_arr) if rho_arr is not None else None, bad, max_listed,
                           C.byref(rep))
    if st != B.G16_OK:
        raise G16Error(st, "g16_srs_check failed")
    return SrsReport(rep, bad[:rep.n_listed])


def new_srs(log2_domain: int, device=0, lib: Optional[B.Library] = None) -> Srs:
    """The string of `snarkjs powersoftau new`: every entry a generator (tau = alpha = beta = 1), byte for byte
    trapdoor_srs(log2_domain, (1, 1, 1)).  It is the start of a ceremony, not a usable SRS: contribute_srs
    re-randomises it."""
    return trapdoor_srs(log2_domain, (1, 1, 1), device=device, lib=lib)


def contribute_srs(srs: Srs, secrets=None, device=0, lib: Optional[B.Library] = None) -> Srs:
    """One powers-of-tau contribution on the GPU (g16_srs_contribute), the point arithmetic of `snarkjs powersoftau
    contribute`: tau_g1[i] and tau_g2[i] times t^i, alpha_tau_g1[i] times a t^i, beta_tau_g1[i] times b t^i and
    beta_g2 times b -- the string of (tau, alpha, beta) becomes the string of (tau t, alpha a, beta b).  Returns a
    NEW Srs with its own arrays (len(srs.tau_g1) and the n_tau of srs.to_c() entries); srs is not written;
    power / ceremony_power are carried over.  secrets: (t, a, b) as ints in [1, r), or None: drawn by the library
    from the OS CSPRNG, never returned and wiped before the call returns.
    The .ptau contribution transcript (challenge hashes, proofs of knowledge of t, a, b, beacon mode) is NOT
    produced, and nothing proves that the result was derived from srs: without the transcript any consistent
    string is a rescaling of any other.  check_srs on the result is the whole of what the points alone can tell."""
    lib = lib or B.load()
    d = srs.to_c()
    sec = None
    if secrets is not None:
        secrets = [int(x) for x in secrets]
        if len(secrets) != 3:
            raise G16Error(B.G16_ERR_INVALID, "secrets = (t, a, b)")
        if any(not 0 < x < FR_MODULUS for x in secrets):
            raise G16Error(B.G16_ERR_INVALID, "t, a and b are integers in [1, r)")
        sec = fr_from_ints(secrets, lib)
    tau_g1 = np.empty((d.n_tau_g1, 64), dtype=np.uint8)
    tau_g2 = np.empty((d.n_tau, 128), dtype=np.uint8)
    alpha = np.empty((d.n_tau, 64), dtype=np.uint8)
    beta = np.empty((d.n_tau, 64), dtype=np.uint8)
    beta_g2 = (C.c_uint8 * 128)()
    st = lib.g16_srs_contribute(device, C.byref(d), _np_ptr(sec) if sec is not None else None, _np_ptr(tau_g1),
                                _np_ptr(tau_g2), _np_ptr(alpha), _np_ptr(beta), beta_g2)
    if st != B.G16_OK:
        raise G16Error(st, "g16_srs_contribute failed")
    out = Srs(tau_g1, tau_g2, alpha, beta, bytes(beta_g2))
    out.power, out.ceremony_power = srs.power, srs.ceremony_power
    return out


SRS_CONTRIBUTE_PHASES = ("upload", "scalars", "mul_g1", "mul_g2", "affine", "download")


def contribute_srs_times(lib: Optional[B.Library] = None) -> dict:
    """milliseconds of device time per phase of this thread's last contribute_srs, summed over the chunks
    (g16_srs_contribute_times); the copies run under the kernels, so the sum exceeds the wall time"""
    return _phase_times(lib, "g16_srs_contribute_times", SRS_CONTRIBUTE_PHASES)


SETUP_SRS_PHASES = ("upload", "ntt_g1", "ntt_g2", "ntt_h", "affine", "combine", "download")


def setup_from_srs_times(lib: Optional[B.Library] = None) -> dict:
    """milliseconds per phase of this thread's last setup_from_srs (g16_setup_from_srs_times)"""
    return _phase_times(lib, "g16_setup_from_srs_times", SETUP_SRS_PHASES)


class CircuitBindingReport:
    """check_key_circuit's verdict.  failed: None, or the first part that did not hold -- "shape" (sizes),
    "gamma_abc_g1" (IC), "gamma_g2", "contribution" (see .contribution, the ContributionReport of the fresh
    key against the key under test; None when an earlier part failed)."""

    def __init__(self, failed, contribution=None):
        self.failed, self.contribution = failed, contribution
        self.ok = failed is None

    def describe(self) -> str:
        if self.ok:
            return "ok"
        if self.failed == "contribution":
            return "not a delta contribution to the circuit's initial key: " + self.contribution.describe()
        return f"{self.failed} differs from the circuit's initial key"

    def __repr__(self):
        return f"CircuitBindingReport({self.describe()})"


def check_key_circuit(pk: "ProvingKey", a: Csr, b: Csr, c: Csr, srs: Srs, rho=None, device=0, max_listed=64,
                      lib: Optional[B.Library] = None, reduction: str = "circom",
                      lagrange: Optional[LagrangeSrs] = None) -> CircuitBindingReport:
    """Is pk a key of THIS circuit under THIS ceremony -- the binding check_key cannot give.  Recomputes the
    initial key from the SRS and the matrices (setup_from_srs), then requires, in this order, vk.gamma_abc_g1
    and vk.gamma_g2 equal to the fresh key's, and check_contribution(fresh, pk).ok: a_query, b_g1_query,
    b_g2_query, alpha and beta byte for byte, l_query, h_query and delta by pairings.  pk should have passed
    check_key; rho, max_listed as check_contribution takes them.
    lagrange: the string's LagrangeSrs; the initial key is then read from it (setup_from_srs(lagrange=...)), with
    the H query of `snarkjs zkey new`.  A key snarkjs made for a circuit smaller than the ceremony passes only
    this way: the default's H query is the reference's, a different set of points for the same proofs, and the
    pairing comparison of h_query reports "contribution"."""
    lib = lib or B.load()
    fresh = setup_from_srs(a, b, c, pk.n_vars, pk.n_public, srs, device=device, lib=lib, reduction=reduction,
                           lagrange=lagrange)
    if fresh.domain_size != pk.domain_size:
        return CircuitBindingReport("shape")
    if not np.array_equal(np.asarray(fresh.vk.gamma_abc_g1), np.asarray(pk.vk.gamma_abc_g1)):
        return CircuitBindingReport("gamma_abc_g1")
    if bytes(fresh.vk.gamma_g2) != bytes(pk.vk.gamma_g2):
        return CircuitBindingReport("gamma_g2")
    rep = check_contribution(fresh, pk, rho=rho, device=device, max_listed=max_listed, lib=lib)
    return CircuitBindingReport(None if rep.ok else "contribution", rep)


# ---- arkworks serialization (include/g16_amd.h) ---------------------------------------------------------------
def _ark_flags(compressed, validate=False) -> int:
    return (B.ARK_COMPRESSED if compressed else 0) | (B.ARK_VALIDATE if validate else 0)


def _ark_group(group) -> int:
    g = {"g1": B.POINT_G1, "g2": B.POINT_G2}.get(group, group) if isinstance(group, str) else int(group)
    if g not in (B.POINT_G1, B.POINT_G2):
        raise G16Error(B.G16_ERR_INVALID, "group is 'g1' or 'g2'")
    return g


def ark_point_bytes(group, compressed=True) -> int:
    """bytes of one ark-serialize'd point: G1 32 / 64, G2 64 / 128"""
    return (64 if _ark_group(group) == B.POINT_G2 else 32) * (1 if compressed else 2)


def _strided(data, n, rec, stride, what):
    """(uint8 array, n) of n records of rec bytes, stride bytes apart (0 = dense)"""
    buf = np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else \
        np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
    step = stride or rec
    if step < rec:
        raise G16Error(B.G16_ERR_INVALID, f"{what}: stride below the record size")
    if n is None:
        if stride not in (0, rec) or buf.shape[0] % rec:
            raise G16Error(B.G16_ERR_INVALID, f"{what}: give n with a stride, or a whole number of records")
        n = buf.shape[0] // rec
    if n and buf.shape[0] < (n - 1) * step + rec:
        raise G16Error(B.G16_ERR_INVALID, f"{what}: {buf.shape[0]} bytes do not hold {n} records")
    return buf, n


def points_from_ark(data, group, n=None, compressed=True, validate=True, in_stride=0, out_stride=0, out=None, device=0,
                    lib: Optional[B.Library] = None):
    """G1Affine / G2Affine::deserialize_with_mode of n points on the GPU (g16_points_from_ark): ark-serialize bytes ->
    (points, reasons, n_bad).  points: the packed Montgomery records of the rest of the package ((n, 64 | 128) uint8,
    or `out` / a flat array when out_stride is given); reasons: n bytes, 0 or the FIRST failed test (B.KEY_BAD_*:
    ENCODING, NONCANONICAL, OFF_CURVE, SUBGROUP with validate on G2); a bad point's record is all-zero."""
    lib = lib or B.load()
    g = _ark_group(group)
    rec_in, rec_out = ark_point_bytes(g, compressed), 128 if g == B.POINT_G2 else 64
    buf, n = _strided(data, n, rec_in, in_stride, "points_from_ark")
    step = out_stride or rec_out
    if step < rec_out:
        raise G16Error(B.G16_ERR_INVALID, "points_from_ark: out_stride below the record size")
    if out is None:
        out = np.zeros((n, rec_out) if step == rec_out else (max(n, 1) - 1) * step + rec_out, dtype=np.uint8)
    elif out.dtype != np.uint8 or not out.flags.c_contiguous or (n and out.size < (n - 1) * step + rec_out):
        raise G16Error(B.G16_ERR_INVALID, "points_from_ark: out must be a contiguous uint8 array that holds n records")
    why = np.zeros(n, dtype=np.uint8)
    bad = C.c_uint64()
    st = lib.g16_points_from_ark(device, g, _ark_flags(compressed, validate), _np_ptr(buf), in_stride, n, _np_ptr(out),
                                 out_stride, _np_ptr(why), C.byref(bad))
    if st != B.G16_OK:
        raise G16Error(st, "g16_points_from_ark failed")
    return out, why, bad.value


def points_to_ark(points, group, n=None, compressed=True, in_stride=0, out_stride=0, out=None, device=0,
                  lib: Optional[B.Library] = None):
    """serialize_with_mode of n packed points on the GPU (g16_points_to_ark) -> uint8 array of ark-serialize records.
    The points are not tested for the curve; a stored word >= q raises G16Error (status G16_ERR_INVALID)."""
    lib = lib or B.load()
    g = _ark_group(group)
    rec_in, rec_out = 128 if g == B.POINT_G2 else 64, ark_point_bytes(g, compressed)
    buf, n = _strided(points, n, rec_in, in_stride, "points_to_ark")
    step = out_stride or rec_out
    if step < rec_out:
        raise G16Error(B.G16_ERR_INVALID, "points_to_ark: out_stride below the record size")
    if out is None:
        out = np.zeros((max(n, 1) - 1) * step + rec_out if n else 0, dtype=np.uint8)
    elif out.dtype != np.uint8 or not out.flags.c_contiguous or (n and out.size < (n - 1) * step + rec_out):
        raise G16Error(B.G16_ERR_INVALID, "points_to_ark: out must be a contiguous uint8 array that holds n records")
    bad = C.c_uint64()
    st = lib.g16_points_to_ark(device, g, _ark_flags(compressed), _np_ptr(buf), in_stride, n, _np_ptr(out), out_stride,
                               C.byref(bad))
    if st != B.G16_OK:
        raise G16Error(st, f"g16_points_to_ark failed: {bad.value} point(s) with a word >= q" if bad.value
                       else "g16_points_to_ark failed")
    return out


def _blob(src) -> np.ndarray:
    if isinstance(src, (bytes, bytearray, memoryview)):
        return np.frombuffer(bytes(src), dtype=np.uint8)
    with open(src, "rb") as f:
        return np.frombuffer(f.read(), dtype=np.uint8)


def _vk_desc(vk: "VerifyingKey"):
    ic = np.ascontiguousarray(vk.gamma_abc_g1, dtype=np.uint8).reshape(-1, 64)
    d = B.VkDesc()
    C.memmove(d.alpha_g1, bytes(vk.alpha_g1), 64)
    C.memmove(d.beta_g2, bytes(vk.beta_g2), 128)
    C.memmove(d.gamma_g2, bytes(vk.gamma_g2), 128)
    C.memmove(d.delta_g2, bytes(vk.delta_g2), 128)
    d.ic, d.ic_count = ic.ctypes.data, ic.shape[0]
    return d, ic


def read_ark_key(src, compressed=True, validate=True, device=0, lib: Optional[B.Library] = None) -> ProvingKey:
    """ProvingKey::<Bn254>::deserialize_compressed / _uncompressed (path or bytes) with the points decoded on the GPU
    (g16_ark_pk_read).  n_vars = len(a_query), n_public = len(gamma_abc_g1) - 1, domain_size = the smallest power of
    two >= len(h_query); h_query comes back padded with infinity to domain_size (a libsnark key has one point less;
    the degenerate libsnark key of domain 2 has ONE H point and comes back with domain_size 1).
    validate: the subgroup test of the G2 points (range and curve are always tested).  A malformed blob or a point
    that fails to decode raises SerializationError (status G16_ERR_IO) naming the array, the index and the reason."""
    lib = lib or B.load()
    buf = _blob(src)
    h = C.c_void_p()
    lib.check(lib.g16_ark_pk_read(device, _ark_flags(compressed, validate), _np_ptr(buf), buf.shape[0], C.byref(h)),
              loader=True)
    handle = _Handle(lib, h, lib.g16_ark_pk_close)
    kd, vd = B.KeyDesc(), B.VkDesc()
    lib.check(lib.g16_ark_pk_key(h, C.byref(kd), C.byref(vd)), loader=True)
    N, p, n = kd.n_vars, kd.n_public, kd.domain_size

    vk = VerifyingKey(bytes(vd.alpha_g1), bytes(vd.beta_g2), bytes(vd.gamma_g2), bytes(vd.delta_g2),
                      _view(vd.ic, vd.ic_count, 64).copy())
    return ProvingKey(N, p, n, vk, bytes(kd.beta_g1), bytes(kd.delta_g1), _view(kd.a_query, N, 64),
                      _view(kd.b_g1_query, N, 64), _view(kd.b_g2_query, N, 128), _view(kd.l_query, N - p - 1, 64),
                      _view(kd.h_query, n, 64), keepalive=handle)


def write_ark_key(pk: ProvingKey, compressed=True, h_len=None, device=0, lib: Optional[B.Library] = None) -> bytes:
    """ProvingKey::serialize_compressed / _uncompressed (g16_ark_pk_write).  h_len: points of h_query to write
    (default domain_size; domain_size - 1 for a key of LibsnarkReduction, so that it round-trips to the same bytes)."""
    lib = lib or B.load()
    h_len = pk.domain_size if h_len is None else int(h_len)
    flags = _ark_flags(compressed)
    kd = pk.to_c()
    vd, _ic = _vk_desc(pk.vk)
    out = np.zeros(lib.g16_ark_pk_size(flags, pk.n_vars, pk.n_public, h_len), dtype=np.uint8)
    lib.check(lib.g16_ark_pk_write(device, flags, C.byref(kd), C.byref(vd), h_len, _np_ptr(out), out.shape[0]),
              loader=True)
    return out.tobytes()


def read_ark_vk(src, compressed=True, validate=True, device=0, lib: Optional[B.Library] = None) -> VerifyingKey:
    """VerifyingKey::<Bn254>::deserialize_compressed / _uncompressed (g16_ark_vk_read)."""
    lib = lib or B.load()
    buf = _blob(src)
    flags = _ark_flags(compressed, validate)
    lay = B.ArkLayout()
    lib.check(lib.g16_ark_vk_layout(_np_ptr(buf), buf.shape[0], flags, C.byref(lay)), loader=True)
    ic = np.zeros((lay.count[4], 64), dtype=np.uint8)
    vd = B.VkDesc()
    lib.check(lib.g16_ark_vk_read(device, flags, _np_ptr(buf), buf.shape[0], C.byref(vd), _np_ptr(ic), ic.shape[0]),
              loader=True)
    return VerifyingKey(bytes(vd.alpha_g1), bytes(vd.beta_g2), bytes(vd.gamma_g2), bytes(vd.delta_g2), ic)


def write_ark_vk(vk: VerifyingKey, compressed=True, device=0, lib: Optional[B.Library] = None) -> bytes:
    """VerifyingKey::serialize_compressed / _uncompressed (g16_ark_vk_write)."""
    lib = lib or B.load()
    flags = _ark_flags(compressed)
    vd, ic = _vk_desc(vk)
    out = np.zeros(lib.g16_ark_vk_size(flags, ic.shape[0] - 1), dtype=np.uint8)
    lib.check(lib.g16_ark_vk_write(device, flags, C.byref(vd), _np_ptr(out), out.shape[0]), loader=True)
    return out.tobytes()


def proofs_from_ark(blob, n=None, compressed=True, validate=True, device=0, lib: Optional[B.Library] = None) -> List[Proof]:
    """n x Proof::deserialize_compressed / _uncompressed (128 / 256 bytes each) on the GPU (g16_ark_proofs_read).
    A point that fails to decode raises SerializationError naming the proof, the point and the reason."""
    lib = lib or B.load()
    rec = 128 if compressed else 256
    buf, n = _strided(blob, n, rec, 0, "proofs_from_ark")
    out = np.zeros(n * B.G16_PROOF_BYTES, dtype=np.uint8)
    why = np.zeros((n, 3), dtype=np.uint8)
    bad = C.c_uint64()
    lib.check(lib.g16_ark_proofs_read(device, _ark_flags(compressed, validate), _np_ptr(buf), n, _np_ptr(out),
                                      _np_ptr(why), C.byref(bad)), loader=True)
    raw = out.tobytes()
    return [Proof(raw[i * B.G16_PROOF_BYTES:(i + 1) * B.G16_PROOF_BYTES]) for i in range(n)]


def proofs_to_ark(proofs, compressed=True, device=0, lib: Optional[B.Library] = None) -> bytes:
    """n x Proof::serialize_compressed / _uncompressed, concatenated (g16_ark_proofs_write)."""
    lib = lib or B.load()
    raw = b"".join(p.raw if isinstance(p, Proof) else bytes(p) for p in proofs)
    n = len(raw) // B.G16_PROOF_BYTES
    buf = np.frombuffer(raw, dtype=np.uint8)
    out = np.zeros(n * (128 if compressed else 256), dtype=np.uint8)
    bad = C.c_uint64()
    st = lib.g16_ark_proofs_write(device, _ark_flags(compressed), _np_ptr(buf), n, _np_ptr(out), C.byref(bad))
    if st != B.G16_OK:
        raise G16Error(st, f"g16_ark_proofs_write failed ({bad.value} point(s) with a word >= q)")
    return out.tobytes()


def _verify_args(vk, proofs, public_inputs, lib):
    """(vk descriptor, proof bytes, Montgomery public inputs, n, keepalive) as the verify entry points take them"""
    raw = b"".join(p.raw if isinstance(p, Proof) else bytes(p) for p in proofs)
    n = len(raw) // B.G16_PROOF_BYTES
    ic = np.ascontiguousarray(vk.gamma_abc_g1, dtype=np.uint8).reshape(-1, 64)
    n_pub = ic.shape[0] - 1
    if len(public_inputs) != n:
        raise G16Error(B.G16_ERR_INVALID, "one public-input vector per proof")
    flat = []
    for pi in public_inputs:
        if len(pi) != n_pub:
            raise G16Error(B.G16_ERR_INVALID, "MalformedVerifyingKey: wrong number of public inputs")
        flat.extend(pi)
    pubs = _as_fr(flat, lib) if (flat and not isinstance(flat[0], np.ndarray)) else \
        (np.ascontiguousarray(np.stack(flat)) if flat else np.zeros((0, 4), np.uint64))
    d = B.VkDesc()
    C.memmove(d.alpha_g1, bytes(vk.alpha_g1), 64)
    C.memmove(d.beta_g2, bytes(vk.beta_g2), 128)
    C.memmove(d.gamma_g2, bytes(vk.gamma_g2), 128)
    C.memmove(d.delta_g2, bytes(vk.delta_g2), 128)
    d.ic, d.ic_count = ic.ctypes.data, ic.shape[0]
    buf = np.frombuffer(raw, dtype=np.uint8)
    return d, buf, pubs, n, ic


class KeyReport(_CheckReport):
    """g16_key_report + the bad-point list of g16_key_check.  ok: no bad point and no failed relation;
    relations_checked: False when a structural failure made the pairing relations meaningless;
    relations_failed: KEY_PAIR_BETA | KEY_PAIR_DELTA | KEY_PAIR_B | KEY_VK_MISMATCH bits (_binding);
    n_points / n_bad / n_infinity: dicts by query name (_binding.KEY_QUERIES);
    bad: [(query_name, index, reason_bits)] in ascending (query, index) order, at most max_listed."""
    RELATIONS = ((B.KEY_PAIR_BETA, "e(beta_g1, g2) != e(g1, beta_g2)"),
                 (B.KEY_PAIR_DELTA, "e(delta_g1, g2) != e(g1, delta_g2)"),
                 (B.KEY_PAIR_B, "b_g1_query and b_g2_query do not hold the same scalars"),
                 (B.KEY_VK_MISMATCH, "the verifying key differs from the proving key"))
    SINGLES = B.KEY_SINGLES

    def __init__(self, rep: B.KeyReportC, bad):
        self._fill(rep, B.KEY_QUERIES)
        self.bad = [(B.KEY_QUERIES[b.query], int(b.index), int(b.reason)) for b in bad]


def check_key(pk: "ProvingKey", vk=None, rho=None, device=0, max_listed=64,
              lib: Optional[B.Library] = None) -> KeyReport:
    """Validation of a proving key on the GPU (g16_key_check): every point of every query canonical, on
    its curve and (G2) in the prime-order subgroup; then e(beta_g1, g2) = e(g1, beta_g2), the same for
    delta, and e(sum rho_i B1_i, g2) = e(g1, sum rho_i B2_i).  Call it once after read_zkey on a key you
    did not mint.  A passing report means the key is well formed and internally consistent, NOT that it
    belongs to your circuit: check_key_circuit ties it to the matrices through the ceremony's powers of tau.
    vk: None = pk.vk, False = skip the verifying-key part (IC, gamma_g2, the byte comparison).
    rho: None (drawn by the library from the OS CSPRNG) or n_vars ints in [1, 2^128)."""
    lib = lib or B.load()
    kd = pk.to_c()
    if vk is None:
        vk = pk.vk
    d = None
    if vk is not False:
        ic = np.ascontiguousarray(vk.gamma_abc_g1, dtype=np.uint8).reshape(-1, 64)
        d = B.VkDesc()
        C.memmove(d.alpha_g1, bytes(vk.alpha_g1), 64)
        C.memmove(d.beta_g2, bytes(vk.beta_g2), 128)
        C.memmove(d.gamma_g2, bytes(vk.gamma_g2), 128)
        C.memmove(d.delta_g2, bytes(vk.delta_g2), 128)
        d.ic, d.ic_count = ic.ctypes.data, ic.shape[0]
    rho_arr = _rho_array(rho, pk.n_vars, "one coefficient per wire")
    max_listed = int(max_listed)
    bad = (B.KeyBadPoint * max(max_listed, 1))()
    rep = B.KeyReportC()
    st = lib.g16_key_check(device, C.byref(kd), C.byref(d) if d is not None else None,
                           _np_ptr(rho_arr) if rho_arr is not None else None, bad, max_listed, C.byref(rep))
    if st != B.G16_OK:
        raise G16Error(st, "g16_key_check failed")
    return KeyReport(rep, bad[:rep.n_listed])


def contribute_key(pk: "ProvingKey", d=None, device=0, lib: Optional[B.Library] = None) -> "ProvingKey":
    """One phase-2 contribution on the GPU (g16_key_contribute): delta_g1 and delta_g2 times d, every point of
    l_query and h_query times d^-1 -- the key of (tau, alpha, beta, gamma, delta) becomes the key of
    (tau, alpha, beta, gamma, delta * d).  Returns a NEW ProvingKey with new l_query, h_query, delta_g1 and
    vk.delta_g2; a_query, b_g1_query, b_g2_query and vk.gamma_abc_g1 are shared with pk.  write_zkey takes it
    as it is.  d: an int in [1, r), or None: drawn by the library from the OS CSPRNG and never returned.
    The snarkjs contribution transcript (challenge hash, proof of knowledge of d) is NOT produced."""
    lib = lib or B.load()
    kd = pk.to_c()
    d_arr = None
    if d is not None:
        d = int(d)
        if not 0 < d < FR_MODULUS:
            raise G16Error(B.G16_ERR_INVALID, "d is an integer in [1, r)")
        d_arr = fr_from_ints([d], lib)
    l_out = np.empty((pk.n_vars - pk.n_public - 1, 64), dtype=np.uint8)
    h_out = np.empty((pk.domain_size, 64), dtype=np.uint8)
    d1, d2 = (C.c_uint8 * 64)(), (C.c_uint8 * 128)()
    st = lib.g16_key_contribute(device, C.byref(kd), _np_ptr(d_arr) if d_arr is not None else None,
                                _np_ptr(l_out), _np_ptr(h_out), d1, d2)
    if st != B.G16_OK:
        raise G16Error(st, "g16_key_contribute failed")
    vk = VerifyingKey(pk.vk.alpha_g1, pk.vk.beta_g2, pk.vk.gamma_g2, bytes(d2), pk.vk.gamma_abc_g1)
    return ProvingKey(pk.n_vars, pk.n_public, pk.domain_size, vk, pk.beta_g1, bytes(d1), pk.a_query,
                      pk.b_g1_query, pk.b_g2_query, l_out, h_out, keepalive=pk)


class ContributionReport(_CheckReport):
    """g16_contribution_report + the bad-point list of g16_key_contribution_check.  ok: nothing but delta
    changed, no bad point, no failed relation; relations_checked: False when a structural failure (or keys of
    different sizes) made the pairing relations meaningless; relations_failed: CONTRIB_* bits (_binding);
    n_bad: {"l_query", "h_query"} counts; bad: [(query_name, index, reason_bits)] in ascending (query, index)
    order, at most max_listed ("singles" index 2 = delta_g1, 4 = delta_g2)."""
    RELATIONS = ((B.CONTRIB_UNCHANGED_MISMATCH, "something other than delta, l_query and h_query differs"),
                 (B.CONTRIB_DELTA_INFINITE, "delta is the point at infinity"),
                 (B.CONTRIB_PAIR_DELTA, "e(delta_g1', g2) != e(g1, delta_g2')"),
                 (B.CONTRIB_PAIR_L, "l_query was not scaled by the inverse of delta's factor"),
                 (B.CONTRIB_PAIR_H, "h_query was not scaled by the inverse of delta's factor"))

    SINGLES = B.KEY_SINGLES

    def __init__(self, rep: B.ContributionReportC, bad):
        self._fill(rep)
        self.n_bad = {"l_query": int(rep.n_bad_l), "h_query": int(rep.n_bad_h)}
        self.bad = [(B.KEY_QUERIES[b.query], int(b.index), int(b.reason)) for b in bad]

    def _bad_words(self):
        return f"{len(self.bad)} bad point(s) listed"

    def _unlisted_words(self):
        if self.relations_failed:
            return self._relation_words()
        return f"{sum(self.n_bad.values())} bad point(s)"


def check_contribution(before: "ProvingKey", after: "ProvingKey", rho=None, device=0, max_listed=64,
                       lib: Optional[B.Library] = None) -> ContributionReport:
    """Is `after` the key `before` with only delta re-randomised (g16_key_contribution_check)?  Bytes of
    everything a contribution leaves alone, structure of after's delta, l_query and h_query, then
    e(delta_g1', g2) = e(g1, delta_g2') and e(sum rho_i L_i, delta_g2) = e(sum rho_i L'_i, delta_g2') for L and
    for H.  `before` should have passed check_key.  vk.gamma_g2 and vk.gamma_abc_g1 are compared here (they are
    not part of the C key descriptor).  rho: None (drawn by the library from the OS CSPRNG) or
    len(l_query) + len(h_query) ints in [1, 2^128), L's first.  The contribution transcript is NOT checked."""
    lib = lib or B.load()
    kb, ka = before.to_c(), after.to_c()
    rho_arr = _rho_array(rho, before.n_vars - before.n_public - 1 + before.domain_size,
                         "one coefficient per point of l_query and h_query")
    max_listed = int(max_listed)
    bad = (B.KeyBadPoint * max(max_listed, 1))()
    rep = B.ContributionReportC()
    st = lib.g16_key_contribution_check(device, C.byref(kb), C.byref(ka),
                                        _np_ptr(rho_arr) if rho_arr is not None else None, bad, max_listed,
                                        C.byref(rep))
    if st != B.G16_OK:
        raise G16Error(st, "g16_key_contribution_check failed")
    out = ContributionReport(rep, bad[:rep.n_listed])
    if bytes(before.vk.gamma_g2) != bytes(after.vk.gamma_g2) or not np.array_equal(
            np.asarray(before.vk.gamma_abc_g1), np.asarray(after.vk.gamma_abc_g1)):
        out.relations_failed |= B.CONTRIB_UNCHANGED_MISMATCH
        out.ok = False
    return out


def verify_batch(vk: "VerifyingKey", proofs, public_inputs, device=0, lib: Optional[B.Library] = None):
    """Groth16::process_vk + verify_with_processed_vk (reference src/zkey.rs:868-870,914-916) for a
    batch under one key on the GPU (g16_verify_batch).  proofs: Proof objects or 256-byte strings;
    public_inputs: one sequence of n_public values (ints or Montgomery rows) per proof.  Returns a
    list of bools."""
    lib = lib or B.load()
    d, buf, pubs, n, _ic = _verify_args(vk, proofs, public_inputs, lib)
    ok = np.zeros(max(n, 1), dtype=np.uint8)
    st = lib.g16_verify_batch(device, C.byref(d), _np_ptr(buf), _np_ptr(pubs), n, _np_ptr(ok))
    if st != B.G16_OK:
        raise G16Error(st, "g16_verify_batch failed")
    return [bool(x) for x in ok[:n]]


def verify_aggregate(vk: "VerifyingKey", proofs, public_inputs, rho=None, device=0,
                     lib: Optional[B.Library] = None, return_structural=False):
    """All proofs of a batch under one key in ONE combined pairing check (g16_verify_aggregate, the
    small-exponent batch test): True iff every proof is well formed and
      prod_i e(rho_i A_i, B_i) = e((sum rho_i) alpha, beta) e(sum rho_i X_i, gamma) e(sum rho_i C_i, delta).
    Inputs as verify_batch takes them.  rho: None (the library draws 128-bit coefficients from the
    operating system's CSPRNG) or one int in [1, 2^128) per proof -- which must be unpredictable to
    whoever made the proofs: a batch with an invalid proof passes with probability <= 2^-127 only then.
    return_structural=True returns (verdict, [proof i is well formed])."""
    lib = lib or B.load()
    d, buf, pubs, n, _ic = _verify_args(vk, proofs, public_inputs, lib)
    rho_arr = _rho_array(rho, n, "one coefficient per proof")
    ok = np.zeros(1, dtype=np.uint8)
    structural = np.zeros(max(n, 1), dtype=np.uint8)
    st = lib.g16_verify_aggregate(device, C.byref(d), _np_ptr(buf), _np_ptr(pubs), n,
                                  _np_ptr(rho_arr) if rho_arr is not None and n else None, _np_ptr(ok),
                                  _np_ptr(structural))
    if st != B.G16_OK:
        raise G16Error(st, "g16_verify_aggregate failed")
    if return_structural:
        return bool(ok[0]), [bool(x) for x in structural[:n]]
    return bool(ok[0])


def verify_batch_fast(vk: "VerifyingKey", proofs, public_inputs, device=0, lib: Optional[B.Library] = None):
    """verify_batch's list at the cost of one aggregate check when every proof is valid (the common
    case): verify_aggregate with fresh coefficients first; if it rejects, the malformed proofs are
    False and the well-formed remainder goes through verify_batch.  Equal to verify_batch's result up
    to the 2^-127 soundness error of the aggregate check."""
    lib = lib or B.load()
    proofs = list(proofs)
    public_inputs = list(public_inputs)
    ok, structural = verify_aggregate(vk, proofs, public_inputs, device=device, lib=lib, return_structural=True)
    if ok:
        return [True] * len(structural)
    rest = [i for i, s in enumerate(structural) if s]
    out = [False] * len(structural)
    if rest:
        for i, v in zip(rest, verify_batch(vk, [proofs[i] for i in rest], [public_inputs[i] for i in rest],
                                           device=device, lib=lib)):
            out[i] = v
    return out


def _verify_groups_args(groups, lib):
    """groups of (vk, proofs, public_inputs) packed as the *_keys entry points take them: (array of vk
    descriptor pointers, counts, proof bytes, public inputs, keepalive)"""
    packed = [_verify_args(vk, proofs, public_inputs, lib) for vk, proofs, public_inputs in groups]
    counts = np.array([p[3] for p in packed], dtype=np.uint32)
    vks = (C.POINTER(B.VkDesc) * max(len(packed), 1))(*[C.pointer(p[0]) for p in packed])
    buf = np.concatenate([p[1] for p in packed]) if packed else np.zeros(0, np.uint8)
    rows = [np.asarray(p[2], dtype=np.uint64).reshape(-1, 4) for p in packed if len(p[2])]
    pubs = np.ascontiguousarray(np.concatenate(rows)) if rows else np.zeros((0, 4), np.uint64)
    return vks, counts, np.ascontiguousarray(buf), pubs, packed


def verify_aggregate_keys(groups, rho=None, device=0, lib: Optional[B.Library] = None, return_structural=False):
    """Proofs under MANY keys in one pass (g16_verify_aggregate_keys).  groups: a sequence of
    (vk, proofs, public_inputs), each as verify_aggregate takes them.  Returns one bool per group: exactly
    verify_aggregate's verdict on that group alone (an empty group is True) -- groups are independent, nothing
    is combined across keys -- for about the cost of ONE verify_aggregate call whatever the number of keys.
    rho: None (drawn by the library) or one list per group, under verify_aggregate's rules.
    return_structural=True returns (verdicts, [[proof i of group k is well formed]])."""
    lib = lib or B.load()
    groups = list(groups)
    vks, counts, buf, pubs, keep = _verify_groups_args(groups, lib)
    n = int(counts.sum())
    rho_arr = None
    if rho is not None:
        rho = [[int(x) for x in r] for r in rho]
        if len(rho) != len(groups) or any(len(r) != c for r, c in zip(rho, counts)):
            raise G16Error(B.G16_ERR_INVALID, "one list of coefficients per group, one coefficient per proof")
        flat = [x for r in rho for x in r]
        if any(not 0 <= x < 1 << 128 for x in flat):
            raise G16Error(B.G16_ERR_INVALID, "coefficients are integers in [1, 2^128)")
        rho_arr = np.array([[x & 0xFFFFFFFFFFFFFFFF, x >> 64] for x in flat], dtype=np.uint64).reshape(n, 2)
    ok = np.zeros(max(len(groups), 1), dtype=np.uint8)
    structural = np.zeros(max(n, 1), dtype=np.uint8)
    st = lib.g16_verify_aggregate_keys(device, vks, _np_ptr(counts), len(groups), _np_ptr(buf), _np_ptr(pubs),
                                       _np_ptr(rho_arr) if rho_arr is not None and n else None, _np_ptr(ok),
                                       _np_ptr(structural))
    if st != B.G16_OK:
        raise G16Error(st, "g16_verify_aggregate_keys failed")
    verdicts = [bool(x) for x in ok[:len(groups)]]
    if return_structural:
        ends = np.cumsum(counts)
        return verdicts, [[bool(x) for x in structural[e - c:e]] for e, c in zip(ends, counts)]
    return verdicts


def verify_batch_keys(groups, device=0, lib: Optional[B.Library] = None):
    """verify_batch for proofs under MANY keys in one pass (g16_verify_batch_keys).  groups as
    verify_aggregate_keys takes them; returns one list of bools per group, verify_batch's on that group."""
    lib = lib or B.load()
    groups = list(groups)
    vks, counts, buf, pubs, keep = _verify_groups_args(groups, lib)
    n = int(counts.sum())
    ok = np.zeros(max(n, 1), dtype=np.uint8)
    st = lib.g16_verify_batch_keys(device, vks, _np_ptr(counts), len(groups), _np_ptr(buf), _np_ptr(pubs),
                                   _np_ptr(ok))
    if st != B.G16_OK:
        raise G16Error(st, "g16_verify_batch_keys failed")
    ends = np.cumsum(counts)
    return [[bool(x) for x in ok[e - c:e]] for e, c in zip(ends, counts)]


def verify_batch_fast_keys(groups, device=0, lib: Optional[B.Library] = None):
    """verify_batch_keys' lists at the cost of one aggregate pass when every proof is valid: ONE
    verify_aggregate_keys call with fresh coefficients; then ONE verify_batch_keys call over the well-formed
    proofs of the rejected groups only (malformed proofs are False).  At most two library calls whatever the
    number of keys; equal to verify_batch_keys up to the 2^-127 soundness error per group."""
    lib = lib or B.load()
    groups = [(vk, list(proofs), list(public_inputs)) for vk, proofs, public_inputs in groups]
    ok, structural = verify_aggregate_keys(groups, device=device, lib=lib, return_structural=True)
    out = [[v] * len(s) for v, s in zip(ok, structural)]
    again = []                                    # (group, indices of its well-formed proofs)
    for k, (v, s) in enumerate(zip(ok, structural)):
        rest = [i for i, w in enumerate(s) if w]
        if not v and rest:
            again.append((k, rest))
    if again:
        sub = [(groups[k][0], [groups[k][1][i] for i in rest], [groups[k][2][i] for i in rest]) for k, rest in again]
        for (k, rest), got in zip(again, verify_batch_keys(sub, device=device, lib=lib)):
            for i, v in zip(rest, got):
                out[k][i] = v
    return out


def _delta_bytes(vk) -> bytes:
    """delta in G2 of a VerifyingKey, or 128 bytes of it"""
    d = bytes(vk.delta_g2) if hasattr(vk, "delta_g2") else bytes(vk)
    if len(d) != 128:
        raise G16Error(B.G16_ERR_INVALID, "vk is a VerifyingKey or the 128 bytes of delta_g2")
    return d


def _rerandomize_scalars(scalars, n, lib):
    """[(r1, r2)] as ints -> (2n, 4) Montgomery rows, refusing what the library would refuse"""
    if scalars is None:
        return None
    scalars = [(int(r1), int(r2)) for r1, r2 in scalars]
    if len(scalars) != n:
        raise G16Error(B.G16_ERR_INVALID, "one (r1, r2) per proof")
    if any(not 0 < r1 < FR_MODULUS or not 0 <= r2 < FR_MODULUS for r1, r2 in scalars):
        raise G16Error(B.G16_ERR_INVALID, "r1 is an integer in [1, r), r2 in [0, r)")
    return fr_from_ints([x for pair in scalars for x in pair], lib) if n else None


def rerandomize_keys(groups, scalars=None, device=0, lib: Optional[B.Library] = None, return_ok=False):
    """Groth16::rerandomize_proof for proofs under MANY keys in one pass (g16_proofs_rerandomize_keys):
      A' = r1^-1 A,  B' = r1 B + (r1 r2) delta,  C' = C + r2 A.
    groups: a sequence of (vk, proofs); vk a VerifyingKey or the 128 bytes of its delta_g2, proofs Proof objects
    or 256-byte strings.  Groups may be empty and a key may appear twice.  scalars: None (every (r1, r2) is drawn
    by the library from the OS CSPRNG, never returned and wiped before the call returns) or one list of (r1, r2)
    ints per group, r1 in [1, r), r2 in [0, r).  Returns one list of Proof per group; return_ok=True returns
    (lists, [[proof i of group k passed the structural tests]]).  A proof that fails them (a coordinate >= q, A or
    C off the curve, B off the twist) comes back as the all-zero record.  The subgroup test of B is NOT applied
    and nothing is verified: the new proof is valid exactly when the old one was -- verify before or after."""
    lib = lib or B.load()
    groups = [(vk, list(proofs)) for vk, proofs in groups]
    raws = [b"".join(p.raw if isinstance(p, Proof) else bytes(p) for p in proofs) for _, proofs in groups]
    if any(len(r) % B.G16_PROOF_BYTES for r in raws):
        raise G16Error(B.G16_ERR_INVALID, "a proof is 256 bytes")
    counts = np.array([len(r) // B.G16_PROOF_BYTES for r in raws], dtype=np.uint32)
    n = int(counts.sum())
    sc = None
    if scalars is not None:
        scalars = [list(s) for s in scalars]
        if len(scalars) != len(groups) or any(len(s) != c for s, c in zip(scalars, counts)):
            raise G16Error(B.G16_ERR_INVALID, "one list of (r1, r2) per group, one pair per proof")
        sc = _rerandomize_scalars([x for s in scalars for x in s], n, lib)
    deltas = np.frombuffer(b"".join(_delta_bytes(vk) for vk, _ in groups), dtype=np.uint8)
    buf = np.frombuffer(b"".join(raws), dtype=np.uint8)
    out = np.zeros(max(n, 1) * B.G16_PROOF_BYTES, dtype=np.uint8)
    ok = np.zeros(max(n, 1), dtype=np.uint8)
    st = lib.g16_proofs_rerandomize_keys(device, _np_ptr(deltas) if len(groups) else None, _np_ptr(counts),
                                         len(groups), _np_ptr(buf) if n else None,
                                         _np_ptr(sc) if sc is not None else None, _np_ptr(out), _np_ptr(ok))
    if st != B.G16_OK:
        raise G16Error(st, "g16_proofs_rerandomize_keys failed")
    raw = out.tobytes()
    ends = [int(e) for e in np.cumsum(counts)]
    res = [[Proof(raw[i * B.G16_PROOF_BYTES:(i + 1) * B.G16_PROOF_BYTES]) for i in range(e - int(c), e)]
           for e, c in zip(ends, counts)]
    if return_ok:
        return res, [[bool(x) for x in ok[e - int(c):e]] for e, c in zip(ends, counts)]
    return res


def rerandomize(vk, proofs, scalars=None, device=0, lib: Optional[B.Library] = None, return_ok=False):
    """Groth16::rerandomize_proof(vk, proof, rng) for a batch under one key on the GPU (g16_proofs_rerandomize),
    one lane per proof:  A' = r1^-1 A,  B' = r1 B + (r1 r2) delta,  C' = C + r2 A.  The result verifies for exactly
    the public inputs the input verifies for and is unlinkable to it; no witness and no proving key are needed.
    vk: a VerifyingKey or the 128 bytes of its delta_g2; proofs: Proof objects or 256-byte strings; scalars: None
    (drawn by the library from the OS CSPRNG, never returned) or one (r1, r2) of ints per proof, r1 in [1, r),
    r2 in [0, r).  Returns a list of Proof; return_ok=True returns (proofs, [passed the structural tests]).
    rerandomize_keys tells what is and what is not tested."""
    lib = lib or B.load()
    proofs = list(proofs)
    raw = b"".join(p.raw if isinstance(p, Proof) else bytes(p) for p in proofs)
    if len(raw) % B.G16_PROOF_BYTES:
        raise G16Error(B.G16_ERR_INVALID, "a proof is 256 bytes")
    n = len(raw) // B.G16_PROOF_BYTES
    sc = _rerandomize_scalars(scalars, n, lib)
    delta = np.frombuffer(_delta_bytes(vk), dtype=np.uint8)
    buf = np.frombuffer(raw, dtype=np.uint8)
    out = np.zeros(max(n, 1) * B.G16_PROOF_BYTES, dtype=np.uint8)
    ok = np.zeros(max(n, 1), dtype=np.uint8)
    st = lib.g16_proofs_rerandomize(device, _np_ptr(delta), _np_ptr(buf) if n else None, n,
                                    _np_ptr(sc) if sc is not None else None, _np_ptr(out), _np_ptr(ok))
    if st != B.G16_OK:
        raise G16Error(st, "g16_proofs_rerandomize failed")
    got = out.tobytes()
    res = [Proof(got[i * B.G16_PROOF_BYTES:(i + 1) * B.G16_PROOF_BYTES]) for i in range(n)]
    if return_ok:
        return res, [bool(x) for x in ok[:n]]
    return res


RERANDOMIZE_PHASES = ("upload", "prepare", "mul_g1", "mul_g2", "affine", "download")


def rerandomize_times(lib: Optional[B.Library] = None) -> dict:
    """milliseconds of device time per phase of this thread's last rerandomize / rerandomize_keys
    (g16_proofs_rerandomize_times): prepare = structural tests + scalars; mul_g1 and mul_g2 run side by side on two
    streams, so the sum exceeds the wall time"""
    return _phase_times(lib, "g16_proofs_rerandomize_times", RERANDOMIZE_PHASES)


class PreparedVerifyingKey:
    """Groth16::process_vk's PreparedVerifyingKey, resident on the device (g16_pvk): the tested key, the Miller value
    of (beta, -alpha) and the line tables of gamma and delta.  prepare_verifying_key makes one; verify_prepared uses
    it; close() (or the garbage collector) releases it."""

    def __init__(self, lib, ptr, n_public, device):
        self.lib, self._ptr, self.n_public, self.device = lib, ptr, n_public, device

    def alpha_beta(self) -> bytes:
        """the stored Miller value of (beta, -alpha): 12 x 32 bytes, coefficient of w^i at 32 i, Montgomery"""
        out = np.zeros(384, dtype=np.uint8)
        self.lib.check(self.lib.g16_pvk_alpha_beta(self._handle(), _np_ptr(out)))
        return out.tobytes()

    def alpha_g1_beta_g2(self) -> "GT":
        """e(alpha_g1, beta_g2), the field of arkworks' PreparedVerifyingKey and snarkjs' vk_alphabeta_12
        (g16_pvk_alpha_g1_beta_g2: paired on first use, then kept in the handle)"""
        out = np.zeros(384, dtype=np.uint8)
        self.lib.check(self.lib.g16_pvk_alpha_g1_beta_g2(self._handle(), _np_ptr(out)))
        return GT(out.tobytes(), self.lib, self.device)

    def _handle(self):
        if not self._ptr:
            raise G16Error(B.G16_ERR_INVALID, "the prepared verifying key is closed")
        return self._ptr

    def close(self):
        if self._ptr:
            self.lib.g16_pvk_destroy(self._ptr)
        self._ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def prepare_verifying_key(vk: "VerifyingKey", device=0, lib: Optional[B.Library] = None) -> PreparedVerifyingKey:
    """Groth16::process_vk(&vk) on the GPU (g16_pvk_create).  The key is TESTED (verify_batch does not): a
    non-canonical coordinate, a point off its curve or a G2 point outside the subgroup raises G16Error
    (G16_ERR_INVALID) naming the point."""
    lib = lib or B.load()
    d, _ic = _vk_desc(vk)
    h = C.c_void_p()
    lib.check(lib.g16_pvk_create(device, C.byref(d), C.byref(h)))
    return PreparedVerifyingKey(lib, h, _ic.shape[0] - 1, device)


def verify_prepared(pvk: PreparedVerifyingKey, proofs, public_inputs):
    """Groth16::verify_with_processed_vk for a batch under a prepared key (g16_verify_prepared): one workgroup per
    proof, the low-latency form.  Arguments and verdicts are verify_batch's.  Returns a list of bools."""
    lib = pvk.lib
    raw = b"".join(p.raw if isinstance(p, Proof) else bytes(p) for p in proofs)
    n = len(raw) // B.G16_PROOF_BYTES
    if len(public_inputs) != n:
        raise G16Error(B.G16_ERR_INVALID, "one public-input vector per proof")
    flat = []
    for pi in public_inputs:
        if len(pi) != pvk.n_public:
            raise G16Error(B.G16_ERR_INVALID, "MalformedVerifyingKey: wrong number of public inputs")
        flat.extend(pi)
    pubs = _as_fr(flat, lib) if (flat and not isinstance(flat[0], np.ndarray)) else \
        (np.ascontiguousarray(np.stack(flat)) if flat else np.zeros((0, 4), np.uint64))
    buf = np.frombuffer(raw, dtype=np.uint8)
    ok = np.zeros(max(n, 1), dtype=np.uint8)
    st = lib.g16_verify_prepared(pvk._handle(), _np_ptr(buf) if n else None, _np_ptr(pubs) if len(flat) else None, n,
                                 _np_ptr(ok))
    if st != B.G16_OK:
        raise G16Error(st, "g16_verify_prepared failed")
    return [bool(x) for x in ok[:n]]


def pairing_check(g1_points, g2_points, device=0, lib: Optional[B.Library] = None) -> bool:
    """prod_i e(P_i, Q_i) == 1 for 1 to 16 pairs on the wave-cooperative pairing (g16_pairing_check).  g1_points:
    64-byte packed G1 points, g2_points: 128-byte packed G2 points (all-zero = infinity: the pair contributes 1).
    A malformed point (non-canonical word, off its curve, Q outside G2) gives False."""
    lib = lib or B.load()
    g1 = np.frombuffer(b"".join(bytes(p) for p in g1_points), dtype=np.uint8)
    g2 = np.frombuffer(b"".join(bytes(q) for q in g2_points), dtype=np.uint8)
    n = len(g1_points)
    if n != len(g2_points) or g1.shape[0] != 64 * n or g2.shape[0] != 128 * n:
        raise G16Error(B.G16_ERR_INVALID, "one 64-byte G1 point per 128-byte G2 point")
    ok = np.zeros(1, dtype=np.uint8)
    st = lib.g16_pairing_check(device, _np_ptr(g1) if n else None, _np_ptr(g2) if n else None, n, _np_ptr(ok))
    if st != B.G16_OK:
        raise G16Error(st, "g16_pairing_check failed: 1 to 16 pairs")
    return bool(ok[0])


def prepare_inputs(pvk: PreparedVerifyingKey, public_inputs) -> List[bytes]:
    """Groth16::prepare_inputs(&pvk, inputs) for a batch (g16_pvk_prepare_inputs): per input vector the point
    X = IC_0 + sum_j pub_j IC_{j+1} as 64 packed bytes (all-zero = infinity) -- the sum verify_prepared forms per proof,
    normalised.  public_inputs: one vector per result, as verify_prepared takes them."""
    lib = pvk.lib
    n = len(public_inputs)
    flat = []
    for pi in public_inputs:
        if len(pi) != pvk.n_public:
            raise G16Error(B.G16_ERR_INVALID, "MalformedVerifyingKey: wrong number of public inputs")
        flat.extend(pi)
    pubs = _as_fr(flat, lib) if (flat and not isinstance(flat[0], np.ndarray)) else \
        (np.ascontiguousarray(np.stack(flat)) if flat else np.zeros((0, 4), np.uint64))
    out = np.zeros(max(n, 1) * 64, dtype=np.uint8)
    st = lib.g16_pvk_prepare_inputs(pvk._handle(), _np_ptr(pubs) if len(flat) else None, n, _np_ptr(out))
    if st != B.G16_OK:
        raise G16Error(st, "g16_pvk_prepare_inputs failed")
    raw = out.tobytes()
    return [raw[64 * i:64 * i + 64] for i in range(n)]


def verify_prepared_inputs(pvk: PreparedVerifyingKey, proofs, prepared) -> List[bool]:
    """Groth16::verify_proof_with_prepared_inputs for a batch (g16_verify_prepared_inputs): verify_prepared with the
    points of prepare_inputs given, so the input ladder is skipped.  The verdicts are verify_prepared's; a prepared
    point with a non-canonical word or off the curve gives False for that proof only."""
    lib = pvk.lib
    raw = b"".join(p.raw if isinstance(p, Proof) else bytes(p) for p in proofs)
    n = len(raw) // B.G16_PROOF_BYTES
    pts = b"".join(bytes(x) for x in prepared)
    if len(prepared) != n or len(pts) != 64 * n:
        raise G16Error(B.G16_ERR_INVALID, "one 64-byte prepared point per proof")
    buf = np.frombuffer(raw, dtype=np.uint8)
    xs = np.frombuffer(pts, dtype=np.uint8)
    ok = np.zeros(max(n, 1), dtype=np.uint8)
    st = lib.g16_verify_prepared_inputs(pvk._handle(), _np_ptr(buf) if n else None, _np_ptr(xs) if n else None, n,
                                        _np_ptr(ok))
    if st != B.G16_OK:
        raise G16Error(st, "g16_verify_prepared_inputs failed")
    return [bool(x) for x in ok[:n]]


# ---- pairing values ----------------------------------------------------------------------------------------------
FQ_MODULUS = 21888242871839275222246405745257275088696311157297823662689037894645226208583
GT_BYTES = 384
_GT_ONE = ((1 << 256) % FQ_MODULUS).to_bytes(32, "little") + bytes(GT_BYTES - 32)   # Montgomery 1 at w^0
_GT_REASONS = {B.KEY_BAD_NONCANONICAL: "a coordinate >= q", B.KEY_BAD_SUBGROUP: "not in GT (g^r != 1)"}


def _gt_error(lib, st, what):
    msg = lib.g16_last_error(None).decode() if st == B.G16_ERR_INVALID else ""
    return G16Error(st, msg if what.split(" ")[0] in msg else what)


class GT:
    """An element of GT, the target group of the pairing: an immutable wrapper of the library's 384 flat bytes (12 Fq
    in Montgomery form, the coefficient of w^i of Fq12 = Fq[w] / (w^12 - 18 w^6 + 82) at 32 i).  Values are the ones
    arkworks' Bn254::pairing and snarkjs give (the reduced pairing raised to the hard part's cofactor
    m = 2x(6x^2 + 3x + 1): include/g16_amd.h).  All arithmetic runs on the device (g16_gt_multiexp); equality and hash
    are those of the bytes, which are unique per element.  to_ark / to_snarkjs give the forms other software reads."""
    __slots__ = ("raw", "lib", "device")

    def __init__(self, raw, lib: Optional[B.Library] = None, device=0):
        raw = bytes(raw)
        if len(raw) != GT_BYTES:
            raise G16Error(B.G16_ERR_INVALID, "a GT element is 384 bytes")
        object.__setattr__(self, "raw", raw)
        object.__setattr__(self, "lib", lib)
        object.__setattr__(self, "device", device)

    def __setattr__(self, name, value):
        raise AttributeError("GT is immutable")

    def __delattr__(self, name):
        raise AttributeError("GT is immutable")

    def __eq__(self, other):
        return isinstance(other, GT) and self.raw == other.raw

    def __ne__(self, other):
        return not self == other

    def __hash__(self):
        return hash(self.raw)

    def __bytes__(self):
        return self.raw

    def __repr__(self):
        return "GT(" + self.raw[:8].hex() + "...)"

    @staticmethod
    def one(lib: Optional[B.Library] = None, device=0) -> "GT":
        return GT(_GT_ONE, lib, device)

    def is_one(self) -> bool:
        return self.raw == _GT_ONE

    def __mul__(self, other):
        if not isinstance(other, GT):
            return NotImplemented
        return gt_multiexp([[(self, 1), (other, 1)]], device=self.device, lib=self.lib)[0]

    def __pow__(self, e):
        """self ** e for any int e, reduced mod r (a negative e included: in GT the inverse is the (r - 1)-th power)"""
        if isinstance(e, bool) or not isinstance(e, int):
            return NotImplemented
        return gt_multiexp([[(self, e)]], device=self.device, lib=self.lib)[0]

    def inverse(self) -> "GT":
        return self ** -1

    def to_ark(self) -> bytes:
        """ark-ff's Fq12::serialize: 12 canonical little-endian Fq in tower order (g16_gt_to_ark)"""
        lib = self.lib or B.load()
        src = np.frombuffer(self.raw, dtype=np.uint8)
        out = np.zeros(GT_BYTES, dtype=np.uint8)
        st = lib.g16_gt_to_ark(self.device, _np_ptr(src), 1, _np_ptr(out))
        if st != B.G16_OK:
            raise G16Error(st, "g16_gt_to_ark failed")
        return out.tobytes()

    @staticmethod
    def from_ark(b, validate=True, lib: Optional[B.Library] = None, device=0) -> "GT":
        """the inverse (g16_gt_from_ark).  G16Error: a coordinate >= q or, with validate, an element outside GT"""
        return gt_from_ark(b, validate=validate, lib=lib, device=device)[0]

    def to_snarkjs(self):
        """snarkjs' JSON form: [2][3][2] decimal strings, Fq12.c_i / Fq6.c_j / Fq2.c_k"""
        a = self.to_ark()
        word = lambda k: str(int.from_bytes(a[32 * k:32 * k + 32], "little"))   # noqa: E731
        return [[[word(2 * (3 * c + v)), word(2 * (3 * c + v) + 1)] for v in range(3)] for c in range(2)]

    @staticmethod
    def from_snarkjs(j, validate=True, lib: Optional[B.Library] = None, device=0) -> "GT":
        """the inverse.  G16Error: not [2][3][2] decimal strings, a coordinate >= q or, with validate, outside GT"""
        try:
            if len(j) != 2 or any(len(c) != 3 or any(len(v) != 2 for v in c) for c in j):
                raise ValueError
            words = [int(w, 10) if isinstance(w, str) else int(w) for c in j for v in c for w in v]
            if any(isinstance(w, bool) for c in j for v in c for w in v) or any(not 0 <= w < 1 << 256 for w in words):
                raise ValueError
        except (TypeError, ValueError):
            raise G16Error(B.G16_ERR_INVALID, "a GT value is [2][3][2] non-negative decimal strings") from None
        return GT.from_ark(b"".join(w.to_bytes(32, "little") for w in words), validate, lib, device)


def gt_from_ark(data, validate=True, lib: Optional[B.Library] = None, device=0) -> List[GT]:
    """n x 384 bytes of ark-serialized Fq12 -> n GT (g16_gt_from_ark, one call).  G16Error names the first refused
    element and the reason: a coordinate >= q or, with validate, g^r != 1."""
    lib = lib or B.load()
    data = bytes(data)
    if len(data) % GT_BYTES:
        raise G16Error(B.G16_ERR_INVALID, "an ark-serialized Fq12 element is 384 bytes")
    n = len(data) // GT_BYTES
    src = np.frombuffer(data, dtype=np.uint8)
    out = np.zeros(max(n, 1) * GT_BYTES, dtype=np.uint8)
    why = np.zeros(max(n, 1), dtype=np.uint8)
    st = lib.g16_gt_from_ark(device, _np_ptr(src) if n else None, n, 1 if validate else 0, _np_ptr(out), _np_ptr(why))
    if st != B.G16_OK:
        raise G16Error(st, "g16_gt_from_ark failed")
    bad = np.flatnonzero(why[:n])
    if len(bad):
        i = int(bad[0])
        raise G16Error(B.G16_ERR_INVALID, f"GT element {i}: {_GT_REASONS.get(int(why[i]), 'rejected')}")
    raw = out.tobytes()
    return [GT(raw[GT_BYTES * i:GT_BYTES * (i + 1)], lib, device) for i in range(n)]


def gt_multiexp(groups, device=0, lib: Optional[B.Library] = None) -> List[GT]:
    """out_i = prod_j g_ij ** s_ij for every group i, a sequence of (GT, int) pairs, in ONE call (g16_gt_multiexp, one
    workgroup per group).  The exponents are reduced mod r here; the elements are taken as members of GT.  An empty
    group gives one."""
    groups = [list(g) for g in groups]
    for g in groups:
        for x, _ in g:
            if not isinstance(x, GT):
                raise G16Error(B.G16_ERR_INVALID, "gt_multiexp takes (GT, int) pairs")
            lib = lib or x.lib
    lib = lib or B.load()
    n = len(groups)
    off = np.zeros(n + 1, dtype=np.uint32)
    off[1:] = np.cumsum([len(g) for g in groups], dtype=np.uint64)
    total = int(off[n])
    elems = np.frombuffer(b"".join(x.raw for g in groups for x, _ in g), dtype=np.uint8)
    sc = np.frombuffer(b"".join((int(e) % FR_MODULUS).to_bytes(32, "little") for g in groups for _, e in g),
                       dtype=np.uint64)
    out = np.zeros(max(n, 1) * GT_BYTES, dtype=np.uint8)
    st = lib.g16_gt_multiexp(device, _np_ptr(elems) if total else None, _np_ptr(sc) if total else None, _np_ptr(off), n,
                             _np_ptr(out))
    if st != B.G16_OK:
        raise _gt_error(lib, st, "g16_gt_multiexp failed")
    raw = out.tobytes()
    return [GT(raw[GT_BYTES * i:GT_BYTES * (i + 1)], lib, device) for i in range(n)]


def pairing_products(groups, device=0, lib: Optional[B.Library] = None, return_ok=False):
    """The VALUES prod_k e(P_k, Q_k) of many products in one call (g16_pairing_products): one workgroup per product,
    0 to 16 pairs each in one Miller loop.  groups: (g1_points, g2_points) per product, 64-byte packed G1 and 128-byte
    packed G2 points (all-zero = infinity: the pair contributes 1; an empty product is one).  A product with a
    malformed point (non-canonical word, off its curve, Q outside G2) comes back as the all-zero element, which is no
    member of GT; return_ok=True returns (values, [well formed]) to tell.  More than 16 pairs in a product raises."""
    lib = lib or B.load()
    groups = [(list(a), list(b)) for a, b in groups]
    n = len(groups)
    if any(len(a) != len(b) for a, b in groups):
        raise G16Error(B.G16_ERR_INVALID, "one 64-byte G1 point per 128-byte G2 point")
    off = np.zeros(n + 1, dtype=np.uint32)
    off[1:] = np.cumsum([len(a) for a, _ in groups], dtype=np.uint64)
    total = int(off[n])
    g1 = np.frombuffer(b"".join(bytes(p) for a, _ in groups for p in a), dtype=np.uint8)
    g2 = np.frombuffer(b"".join(bytes(q) for _, b in groups for q in b), dtype=np.uint8)
    if g1.shape[0] != 64 * total or g2.shape[0] != 128 * total:
        raise G16Error(B.G16_ERR_INVALID, "one 64-byte G1 point per 128-byte G2 point")
    out = np.zeros(max(n, 1) * GT_BYTES, dtype=np.uint8)
    ok = np.zeros(max(n, 1), dtype=np.uint8)
    st = lib.g16_pairing_products(device, _np_ptr(g1) if total else None, _np_ptr(g2) if total else None, _np_ptr(off),
                                  n, _np_ptr(out), _np_ptr(ok))
    if st != B.G16_OK:
        raise _gt_error(lib, st, "g16_pairing_products failed")
    raw = out.tobytes()
    res = [GT(raw[GT_BYTES * i:GT_BYTES * (i + 1)], lib, device) for i in range(n)]
    if return_ok:
        return res, [bool(x) for x in ok[:n]]
    return res


def pairing(p, q, device=0, lib: Optional[B.Library] = None) -> GT:
    """e(p, q) for one packed G1 point and one packed G2 point (pairing_products with one product of one pair); a
    malformed point raises"""
    vals, ok = pairing_products([([p], [q])], device=device, lib=lib, return_ok=True)
    if not ok[0]:
        raise G16Error(B.G16_ERR_INVALID, "pairing: a malformed point (non-canonical, off its curve or outside G2)")
    return vals[0]


GT_PHASES = ("upload", "g2_tests", "kernels", "download")


def gt_times(lib: Optional[B.Library] = None) -> dict:
    """milliseconds of device time per phase of this thread's last pairing_products / gt_multiexp / codec call
    (g16_gt_times); g2_tests runs beside kernels on a second stream"""
    return _phase_times(lib, "g16_gt_times", GT_PHASES)


VERIFY_PREPARED_PHASES = ("upload", "inputs", "g2_tests", "pairing", "download", "prepare")


def verify_prepared_times(lib: Optional[B.Library] = None) -> dict:
    """milliseconds of device time per phase of this thread's last verify_prepared (g16_verify_prepared_times):
    g2_tests runs beside inputs and pairing on a second stream; prepare is the thread's last prepare_verifying_key"""
    return _phase_times(lib, "g16_verify_prepared_times", VERIFY_PREPARED_PHASES)


# ---- MSM over caller-supplied bases, division by (X - z), KZG (include/g16_amd.h) ---------------------------------
GROUP_G1, GROUP_G2 = 0, 1
MSM_SCALARS_CANONICAL, MSM_SCALARS_DEVICE, MSM_POINTS_DEVICE = 1, 2, 4
POLY_RUN, POLY_BLOCK = 8, 256   # G16_POLY_RUN / G16_POLY_BLOCK: coefficients per lane, lanes per block of the division


def _msm_group(group) -> int:
    if group in (0, "g1", "G1"):
        return GROUP_G1
    if group in (1, "g2", "G2"):
        return GROUP_G2
    raise G16Error(B.G16_ERR_INVALID, "group is 'g1' or 'g2'")


def _is_device_tensor(x) -> bool:
    return hasattr(x, "data_ptr") and bool(getattr(x, "is_cuda", False))


def _msm_points(points, group):
    """packed affine points -> (pointer, count, flags, keepalive): an (n, 64 / 128) uint8 array, raw bytes, a list of
    packed points, or a contiguous uint8 device tensor"""
    width = 128 if group == GROUP_G2 else 64
    if _is_device_tensor(points):
        if points.element_size() != 1 or points.numel() % width or not points.is_contiguous():
            raise G16Error(B.G16_ERR_INVALID, f"device points: a contiguous uint8 tensor of {width} bytes per point")
        return C.c_void_p(points.data_ptr()), points.numel() // width, MSM_POINTS_DEVICE, points
    if isinstance(points, (list, tuple)):
        points = b"".join(bytes(p) for p in points)
    if isinstance(points, (bytes, bytearray, memoryview)):
        points = np.frombuffer(bytes(points), dtype=np.uint8)
    a = np.ascontiguousarray(points, dtype=np.uint8)
    if a.size % width:
        raise G16Error(B.G16_ERR_INVALID, f"points: {width} bytes per point")
    a = a.reshape(-1, width)
    return _np_ptr(a), a.shape[0], 0, a


def _msm_scalars(scalars):
    """scalar vectors -> (pointer, len, count, flags, keepalive, batched).  Accepted: ints (a sequence = one vector, a
    sequence of sequences = a batch), canonical little-endian values ((len, 32) / (count, len, 32) uint8 array or
    bytes), Montgomery limbs ((len, 4) / (count, len, 4) uint64 array), and contiguous device tensors of either
    form (uint8 with 32 bytes per value: canonical; 64-bit with 4 words per value: Montgomery)."""
    if _is_device_tensor(scalars):
        t = scalars
        if not t.is_contiguous() or t.dim() not in (2, 3):
            raise G16Error(B.G16_ERR_INVALID, "device scalars: a contiguous (len, w) or (count, len, w) tensor")
        canon = t.element_size() == 1 and t.shape[-1] == 32
        if not canon and not (t.element_size() == 8 and t.shape[-1] == 4):
            raise G16Error(B.G16_ERR_INVALID, "device scalars: uint8 x 32 (canonical) or 64-bit x 4 (Montgomery) per value")
        batched = t.dim() == 3
        return (C.c_void_p(t.data_ptr()), int(t.shape[-2]), int(t.shape[0]) if batched else 1,
                MSM_SCALARS_DEVICE | (MSM_SCALARS_CANONICAL if canon else 0), t, batched)
    if isinstance(scalars, np.ndarray) and scalars.dtype == np.uint64:
        if scalars.ndim not in (2, 3) or scalars.shape[-1] != 4:
            raise G16Error(B.G16_ERR_INVALID, "Montgomery scalars: a (len, 4) or (count, len, 4) uint64 array")
        a = np.ascontiguousarray(scalars)
        return _np_ptr(a), a.shape[-2], a.shape[0] if a.ndim == 3 else 1, 0, a, a.ndim == 3
    if isinstance(scalars, np.ndarray) and scalars.dtype == np.uint8 and scalars.ndim == 3:
        if scalars.shape[-1] != 32:
            raise G16Error(B.G16_ERR_INVALID, "canonical scalars: 32 bytes per value")
        a = np.ascontiguousarray(scalars)
        return _np_ptr(a), a.shape[1], a.shape[0], MSM_SCALARS_CANONICAL, a, True
    if isinstance(scalars, (np.ndarray, bytes, bytearray, memoryview)):
        a = _canonical_bytes(scalars)
        return _np_ptr(a), a.shape[0], 1, MSM_SCALARS_CANONICAL, a, False
    rows = list(scalars)
    if rows and isinstance(rows[0], (list, tuple, np.ndarray)):
        if len({len(r) for r in rows}) != 1:
            raise G16Error(B.G16_ERR_INVALID, "a batch of scalar vectors: every vector of the same length")
        a = np.stack([_canonical_bytes([int(v) for v in r]) for r in rows]) if len(rows[0]) else \
            np.zeros((len(rows), 0, 32), dtype=np.uint8)
        return _np_ptr(a), a.shape[1], a.shape[0], MSM_SCALARS_CANONICAL, a, True
    a = _canonical_bytes([int(v) for v in rows])
    return _np_ptr(a), a.shape[0], 1, MSM_SCALARS_CANONICAL, a, False


class MsmBases:
    """The MSM engine over bases the caller supplies (ark-ec VariableBaseMSM::msm): g16_msm_bases_create.  points:
    packed affine points in the zkey encoding (64 bytes for 'g1', 128 for 'g2'; Montgomery; all-zero = infinity) as
    an array, bytes, a list of packed points or a uint8 device tensor.  planes: stored multiples per point (None: as
    many as fit the device memory, 1: none precomputed); max_batch: scalar vectors summed in one pass; validate: test
    every point first (canonical, on the curve, G2: in the subgroup) -- a bad point raises G16Error naming it."""

    def __init__(self, points, group="g1", planes=None, max_batch=1, validate=False, window_bits=None, device=0,
                 lib: Optional[B.Library] = None):
        self.lib = lib or B.load()
        self.group = _msm_group(group)
        ptr, n, flags, keep = _msm_points(points, self.group)
        opt = B.MsmOptions(int(window_bits or 0), int(planes or 0), int(max_batch), 1 if validate else 0)
        h = C.c_void_p()
        self.lib.check(self.lib.g16_msm_bases_create(device, self.group, ptr, n, flags, C.byref(opt), C.byref(h)))
        self._h = _Handle(self.lib, h, self.lib.g16_msm_bases_destroy)
        self.n = n
        self.point_bytes = 128 if self.group == GROUP_G2 else 64

    def info(self) -> dict:
        out = (C.c_uint32 * 8)()
        self.lib.check(self.lib.g16_msm_bases_info(self._h.ptr, out))
        return dict(zip(("group", "n", "window_bits", "windows", "planes", "bucket_sets", "batch", "validated"),
                        (int(x) for x in out)))

    def msm(self, scalars):
        """sum_i scalars[i] * points[i] over the first len(scalars) bases: the packed affine point (bytes; all-zero =
        infinity).  A 2-D input (a sequence of vectors, a (count, len, w) array or tensor) is a batch: a list of
        points, one per vector."""
        ptr, ln, count, flags, keep, batched = _msm_scalars(scalars)
        out = np.zeros((max(count, 1), self.point_bytes), dtype=np.uint8)
        self.lib.check(self.lib.g16_msm(self._h.ptr, ptr, ln, count, ln, flags, _np_ptr(out)))
        res = [out[k].tobytes() for k in range(count)]
        return res if batched else res[0]

    def close(self):
        self._h.__del__()


def msm(points, scalars, group="g1", device=0, lib: Optional[B.Library] = None) -> bytes:
    """One MSM over bases used once (g16_msm_once; arkworks' G1Projective::msm(bases, scalars)): no planes are
    precomputed and nothing stays on the device.  The packed affine point."""
    lib = lib or B.load()
    g = _msm_group(group)
    pptr, n, pflags, pkeep = _msm_points(points, g)
    sptr, ln, count, sflags, skeep, batched = _msm_scalars(scalars)
    if batched or ln != n:
        raise G16Error(B.G16_ERR_INVALID, "msm: one scalar per point (MsmBases.msm takes batches and shorter vectors)")
    out = np.zeros(128 if g == GROUP_G2 else 64, dtype=np.uint8)
    lib.check(lib.g16_msm_once(device, g, pptr, sptr, n, pflags | sflags, _np_ptr(out)))
    return out.tobytes()


def poly_divide_linear(coeffs, z, device=0, lib: Optional[B.Library] = None):
    """p(X) = q(X) (X - z) + y on the GPU (g16_poly_divide_linear).  coeffs: one polynomial (coefficient of X^i at i)
    or a batch of equally long ones, in any host form MsmBases.msm takes; z: one point per polynomial (ints or
    Montgomery limbs).  Returns (q, y) as ints -- q a list of n - 1 coefficients -- or a list of such pairs for a batch."""
    lib = lib or B.load()
    ptr, n, count, flags, keep, batched = _msm_scalars(coeffs)
    if flags & MSM_SCALARS_DEVICE:
        raise G16Error(B.G16_ERR_INVALID, "poly_divide_linear: host coefficients (KzgKey.open keeps quotients on the device)")
    zs = list(z) if isinstance(z, (list, tuple, np.ndarray)) else [z]
    if isinstance(z, np.ndarray) and z.dtype == np.uint64:
        zarr = np.ascontiguousarray(z).reshape(-1, 4)
        zarr = zarr if not (flags & MSM_SCALARS_CANONICAL) else _canonical_bytes(fr_to_ints(zarr, lib))
    else:
        zarr = _canonical_bytes([int(v) for v in zs]) if flags & MSM_SCALARS_CANONICAL else fr_from_ints(zs, lib)
    if zarr.shape[0] != count:
        raise G16Error(B.G16_ERR_INVALID, "poly_divide_linear: one point z per polynomial")
    quot = np.zeros((count, max(n - 1, 0), 4), dtype=np.uint64)
    rem = np.zeros((count, 4), dtype=np.uint64)
    lib.check(lib.g16_poly_divide_linear(device, ptr, n, count, _np_ptr(zarr), flags, _np_ptr(quot), _np_ptr(rem)))
    ys = fr_to_ints(rem, lib)
    res = [(fr_to_ints(quot[k], lib) if n > 1 else [], ys[k]) for k in range(count)]
    return res if batched else res[0]


KZG_PHASES = ("input", "divide_or_scalars", "msm", "output_or_pairing")


def kzg_times(lib: Optional[B.Library] = None) -> dict:
    """device milliseconds per phase of this thread's last KzgKey.open / kzg_verify (g16_kzg_times)"""
    return _phase_times(lib, "g16_kzg_times", KZG_PHASES)


def _kzg_points(x, what) -> np.ndarray:
    if isinstance(x, (bytes, bytearray, memoryview)):
        x = np.frombuffer(bytes(x), dtype=np.uint8)
    elif isinstance(x, (list, tuple)):
        x = np.frombuffer(b"".join(bytes(p) for p in x), dtype=np.uint8)
    a = np.ascontiguousarray(x, dtype=np.uint8)
    if a.size % 64:
        raise G16Error(B.G16_ERR_INVALID, f"{what}: 64 bytes per G1 point")
    return a.reshape(-1, 64)


def kzg_verify(tau_g2, commitments, z, y, proofs, rho=None, device=0, lib: Optional[B.Library] = None) -> bool:
    """One verdict for a batch of KZG openings (g16_kzg_verify) by a caller that holds only tau_g2 = tau G2 (128
    bytes): e(sum rho_i (C_i - y_i G + z_i pi_i), G2) == e(sum rho_i pi_i, tau G2).  commitments, proofs: packed G1
    points; z, y: ints or Montgomery limbs; rho: None (the library draws 128-bit coefficients) or ints in [1, 2^128)."""
    lib = lib or B.load()
    cm, pf = _kzg_points(commitments, "commitments"), _kzg_points(proofs, "proofs")
    zz, yy = _as_fr(z, lib), _as_fr(y, lib)
    n = cm.shape[0]
    if not (pf.shape[0] == zz.shape[0] == yy.shape[0] == n):
        raise G16Error(B.G16_ERR_INVALID, "kzg_verify: one commitment, point, value and proof per opening")
    t2 = np.frombuffer(bytes(tau_g2), dtype=np.uint8)
    if t2.size != 128:
        raise G16Error(B.G16_ERR_INVALID, "kzg_verify: tau_g2 is one packed G2 point (128 bytes)")
    r = _rho_array(rho, n, "kzg_verify: one coefficient per opening")
    ok = C.c_uint8(0)
    lib.check(lib.g16_kzg_verify(device, _np_ptr(t2), _np_ptr(cm), _np_ptr(zz), _np_ptr(yy), _np_ptr(pf), n,
                                 None if r is None else _np_ptr(r), C.byref(ok)))
    return bool(ok.value)


class KzgKey:
    """A KZG commitment key on a powers-of-tau string (g16_kzg_key_create): the MSM engine over srs.tau_g1[:max_len]
    with precomputed planes, and tau_g2[1].  The string is used as it comes: check_srs verifies one."""

    def __init__(self, srs: Srs, max_len=None, planes=None, max_batch=1, device=0, lib: Optional[B.Library] = None):
        self.lib = lib or B.load()
        self.device = device
        d = srs.to_c()
        opt = B.MsmOptions(0, int(planes or 0), int(max_batch), 0)
        h = C.c_void_p()
        self.lib.check(self.lib.g16_kzg_key_create(device, C.byref(d), int(max_len or 0), C.byref(opt), C.byref(h)))
        self._h = _Handle(self.lib, h, self.lib.g16_kzg_key_destroy)
        self.max_len = int(max_len or srs.tau_g1.shape[0])
        self.tau_g2 = srs.tau_g2[1].tobytes()

    def info(self) -> dict:
        out = (C.c_uint32 * 8)()
        self.lib.check(self.lib.g16_kzg_key_info(self._h.ptr, out))
        return dict(zip(("group", "n", "window_bits", "windows", "planes", "bucket_sets", "batch", "validated"),
                        (int(x) for x in out)))

    def commit(self, coeffs):
        """p(tau) G for one coefficient vector, or a list of commitments for a batch (forms: MsmBases.msm)"""
        ptr, ln, count, flags, keep, batched = _msm_scalars(coeffs)
        out = np.zeros((max(count, 1), 64), dtype=np.uint8)
        self.lib.check(self.lib.g16_kzg_commit(self._h.ptr, ptr, ln, count, ln, flags, _np_ptr(out)))
        res = [out[k].tobytes() for k in range(count)]
        return res if batched else res[0]

    def open(self, coeffs, z):
        """(y, proof) = (p(z) as an int, q(tau) G as 64 bytes) with q = (p - y) / (X - z); a batch of polynomials with
        one z each gives a list of pairs.  The quotients never leave the device."""
        ptr, ln, count, flags, keep, batched = _msm_scalars(coeffs)
        zs = list(z) if isinstance(z, (list, tuple, np.ndarray)) else [z]
        zarr = _canonical_bytes([int(v) for v in zs]) if flags & MSM_SCALARS_CANONICAL else fr_from_ints(zs, self.lib)
        if zarr.shape[0] != count:
            raise G16Error(B.G16_ERR_INVALID, "open: one point z per polynomial")
        y = np.zeros((max(count, 1), 4), dtype=np.uint64)
        pf = np.zeros((max(count, 1), 64), dtype=np.uint8)
        self.lib.check(self.lib.g16_kzg_open(self._h.ptr, ptr, ln, count, ln, _np_ptr(zarr), flags, _np_ptr(y),
                                             _np_ptr(pf)))
        ys = fr_to_ints(y[:count], self.lib)
        res = [(ys[k], pf[k].tobytes()) for k in range(count)]
        return res if batched else res[0]

    def verify(self, commitments, z, y, proofs, rho=None) -> bool:
        """kzg_verify under this key's tau_g2; single values are a batch of one"""
        if isinstance(commitments, (bytes, bytearray)) and len(commitments) == 64 and not isinstance(z, (list, tuple, np.ndarray)):
            z, y = [z], [y]
        return kzg_verify(self.tau_g2, commitments, z, y, proofs, rho=rho, device=self.device, lib=self.lib)

    def close(self):
        self._h.__del__()


class _Reduction:
    """R1CSToQAP::witness_map_from_matrices on the GPU; the subclass names the QAP."""
    NAME = "circom"

    @classmethod
    def witness_map_from_matrices(cls, matrices: ConstraintMatrices, num_inputs: int,
                                  num_constraints: int, full_assignment, lib=None, device=0):
        if num_inputs != matrices.num_instance_variables or num_constraints != matrices.num_constraints:
            raise G16Error(B.G16_ERR_INVALID, "num_inputs/num_constraints do not match the matrices")
        attr = "_wm_prover_" + cls.NAME
        pr = getattr(matrices, attr, None)
        if pr is None:
            n_vars = len(full_assignment)
            pr = Prover(None, matrices, device=device, lib=lib, n_vars=n_vars, reduction=cls.NAME)
            setattr(matrices, attr, pr)
        return pr.witness_map(full_assignment)


class CircomReduction(_Reduction):
    """R1CSToQAP impl used for circom/snarkjs keys (reference src/circom/qap.rs:12-106)."""
    NAME = "circom"


class LibsnarkReduction(_Reduction):
    """ark_groth16::LibsnarkReduction, the default QAP of `Groth16<Bn254>` (arkworks-generated keys,
    reference tests/groth16.rs:9,25-35).  Returns the n coefficients of h."""
    NAME = "libsnark"


class Groth16:
    """Groth16::<Bn254, CircomReduction> entry points of the proving path."""

    @staticmethod
    def _prover(pk: ProvingKey, matrices: ConstraintMatrices, **kw) -> Prover:
        kw.setdefault("reduction", getattr(pk, "reduction", "circom"))
        if pk._prover is None or pk._prover.matrices is not matrices:
            pk._prover = Prover(pk, matrices, **kw)
        return pk._prover

    @staticmethod
    def generate_random_parameters_with_reduction(r1cs: "R1CS", rng=None, reduction: str = "libsnark",
                                                  device=0, lib=None) -> ProvingKey:
        """Groth16::<Bn254, QAP>::generate_random_parameters_with_reduction(circuit, rng) (reference
        tests/groth16.rs:25, QAP defaulting to LibsnarkReduction there): toxic waste from rng, key
        minted on the GPU.  The key remembers its reduction; Groth16.prove uses it."""
        rng = rng or random.SystemRandom()
        toxic = [rng.randrange(1, FR_MODULUS) for _ in range(5)]
        pk = trapdoor_setup(r1cs.a, r1cs.b, r1cs.c, r1cs.num_variables, r1cs.num_inputs - 1, toxic,
                            device=device, lib=lib, reduction=reduction)
        pk.reduction = reduction
        return pk

    @staticmethod
    def verify(vk: "VerifyingKey", public_inputs, proof, **kw) -> bool:
        """Groth16::verify_with_processed_vk(&process_vk(&vk), inputs, &proof) on the GPU"""
        return verify_batch(vk, [proof], [list(public_inputs)], **kw)[0]

    @staticmethod
    def process_vk(vk: "VerifyingKey", **kw) -> PreparedVerifyingKey:
        """Groth16::process_vk(&vk) on the GPU (prepare_verifying_key): the key is tested and its tables built once"""
        return prepare_verifying_key(vk, **kw)

    @staticmethod
    def verify_with_processed_vk(pvk: PreparedVerifyingKey, public_inputs, proof) -> bool:
        """Groth16::verify_with_processed_vk(&pvk, inputs, &proof) on the GPU, one workgroup for the proof"""
        return verify_prepared(pvk, [proof], [list(public_inputs)])[0]

    @staticmethod
    def prepare_inputs(pvk: PreparedVerifyingKey, public_inputs) -> bytes:
        """Groth16::prepare_inputs(&pvk, inputs) on the GPU: IC_0 + sum_j inputs_j IC_{j+1}, 64 packed bytes"""
        return prepare_inputs(pvk, [list(public_inputs)])[0]

    @staticmethod
    def verify_proof_with_prepared_inputs(pvk: PreparedVerifyingKey, proof, prepared_inputs) -> bool:
        """Groth16::verify_proof_with_prepared_inputs(&pvk, &proof, &prepared_inputs) on the GPU"""
        return verify_prepared_inputs(pvk, [proof], [prepared_inputs])[0]

    @staticmethod
    def rerandomize_proof(vk: "VerifyingKey", proof, rng=None, **kw) -> Proof:
        """Groth16::rerandomize_proof(&vk, &proof, rng) on the GPU: r1 != 0 and r2 from rng (anything with
        randrange); rng=None lets the library draw them from the OS CSPRNG.  rerandomize does a batch."""
        scalars = None if rng is None else [(rng.randrange(1, FR_MODULUS), rng.randrange(FR_MODULUS))]
        return rerandomize(vk, [proof], scalars, **kw)[0]

    @staticmethod
    def create_proof_with_reduction_and_matrices(pk: ProvingKey, r, s, matrices: ConstraintMatrices,
                                                 num_inputs: int, num_constraints: int,
                                                 full_assignment, **kw) -> Proof:
        """Argument order of reference benches/groth16.rs:52-60 / src/zkey.rs:903-911."""
        if num_inputs != matrices.num_instance_variables or num_constraints != matrices.num_constraints:
            raise G16Error(B.G16_ERR_INVALID, "num_inputs/num_constraints do not match the matrices")
        return Groth16._prover(pk, matrices, **kw).prove(r, s, full_assignment)

    @staticmethod
    def prove(pk: ProvingKey, matrices: ConstraintMatrices, circuit: CircomCircuit, rng=None, **kw) -> Proof:
        """SNARK::prove(&pk, circuit, rng) (reference src/zkey.rs:866): r, s <- rng, then the matrices
        entry (rebuilding a ConstraintSystem per proof is the serial host work this path avoids)."""
        rng = rng or random.SystemRandom()
        r = rng.randrange(FR_MODULUS)
        s = rng.randrange(FR_MODULUS)
        # the assignment generate_constraints would allocate (circuit.rs:35-58): through the wire
        # mapping when the circuit carries one, so that it matches get_public_inputs()
        w = circuit.full_assignment()
        return Groth16.create_proof_with_reduction_and_matrices(
            pk, r, s, matrices, matrices.num_instance_variables, matrices.num_constraints, w, **kw)


from .snarkjs import (read_proof_json, write_proof_json, read_public_json, write_public_json, read_vk_json,  # noqa: E402
                      write_vk_json, inputs_to_eth, solidity_calldata)
