"""python -m circom_compat_amd -- file to file, in the place of the snarkjs / rapidsnark commands:

    prove <circuit.zkey> <witness.wtns> <proof.json> <public.json>     rapidsnark prover, snarkjs groth16 prove
    prove-batch <circuit.zkey> <outdir> <witness.wtns>...              one batched pass; <stem>.proof.json, <stem>.public.json
    verify [--check-alphabeta] <verification_key.json> <public.json> <proof.json>     snarkjs groth16 verify: OK / INVALID
    export-vkey [--alphabeta] <circuit.zkey> <verification_key.json>   snarkjs zkey export verificationkey
    calldata <public.json> <proof.json>                                snarkjs zkey export soliditycalldata
    wtns-check <circuit.r1cs> <witness.wtns>                           snarkjs wtns check

Exit status: 0 = done (verify: OK, wtns-check: satisfied), 1 = INVALID / an unsatisfied constraint, 2 = bad usage or
bad input, with one line on stderr and no traceback.
"""
from __future__ import annotations

import argparse
import os
import sys

import circom_compat_amd as cc


def _parser():
    p = argparse.ArgumentParser(prog="python -m circom_compat_amd", description="Groth16 (BN254) on the GPU, file to file")
    p.add_argument("--device", type=int, default=0, help="HIP device ordinal (default 0)")
    sub = p.add_subparsers(dest="cmd", required=True)
    s = sub.add_parser("prove", help="prove one witness")
    for a in ("zkey", "wtns", "proof", "public"):
        s.add_argument(a)
    s = sub.add_parser("prove-batch", help="prove many witnesses under one key in one pass")
    s.add_argument("zkey")
    s.add_argument("outdir")
    s.add_argument("wtns", nargs="+")
    s = sub.add_parser("verify", help="verify one proof")
    for a in ("vkey", "public", "proof"):
        s.add_argument(a)
    s.add_argument("--check-alphabeta", action="store_true",
                   help="recompute e(alpha, beta) and compare it with the key's vk_alphabeta_12, if it has one")
    s = sub.add_parser("export-vkey", help="write the verification key of a zkey")
    for a in ("zkey", "vkey"):
        s.add_argument(a)
    s.add_argument("--alphabeta", action="store_true", help="write vk_alphabeta_12 = e(alpha, beta), as snarkjs does")
    s = sub.add_parser("calldata", help="print the arguments of verifyProof")
    for a in ("public", "proof"):
        s.add_argument(a)
    s = sub.add_parser("wtns-check", help="check a witness against the constraints")
    for a in ("r1cs", "wtns"):
        s.add_argument(a)
    return p


def _need(*paths):
    for p in paths:
        if not os.path.isfile(p):
            raise FileNotFoundError(f"{p}: no such file")


def _run(a, lib) -> int:
    dev = a.device
    if a.cmd == "prove":
        _need(a.zkey, a.wtns)
        pk, mats = cc.read_zkey(a.zkey, lib=lib)
        w = cc.open_wtns(a.wtns, lib=lib)
        proof = cc.Prover(pk, mats, device=dev, lib=lib).prove_wtns(w)
        cc.write_proof_json(a.proof, proof, device=dev, lib=lib)
        cc.write_public_json(a.public, w.public_inputs(pk.n_public))
        return 0
    if a.cmd == "prove-batch":
        _need(a.zkey, *a.wtns)
        stems = [os.path.splitext(os.path.basename(p))[0] for p in a.wtns]
        if len(set(stems)) != len(stems):
            raise ValueError("two witness files with the same name")
        pk, mats = cc.read_zkey(a.zkey, lib=lib)
        ws = [cc.open_wtns(p, lib=lib) for p in a.wtns]
        proofs = cc.Prover(pk, mats, device=dev, lib=lib).prove_wtns_batch(ws)
        os.makedirs(a.outdir, exist_ok=True)
        for stem, w, proof in zip(stems, ws, proofs):
            cc.write_proof_json(os.path.join(a.outdir, stem + ".proof.json"), proof, device=dev, lib=lib)
            cc.write_public_json(os.path.join(a.outdir, stem + ".public.json"), w.public_inputs(pk.n_public))
        return 0
    if a.cmd == "verify":
        _need(a.vkey, a.public, a.proof)
        vk = cc.read_vk_json(a.vkey, device=dev, lib=lib, check_alphabeta=a.check_alphabeta)
        ok = cc.verify_batch(vk, [cc.read_proof_json(a.proof, device=dev, lib=lib)], [cc.read_public_json(a.public)],
                             device=dev, lib=lib)[0]
        print("OK" if ok else "INVALID")
        return 0 if ok else 1
    if a.cmd == "export-vkey":
        _need(a.zkey)
        cc.write_vk_json(a.vkey, cc.read_zkey(a.zkey, lib=lib)[0].vk, device=dev, lib=lib, alphabeta=a.alphabeta)
        return 0
    if a.cmd == "calldata":
        _need(a.public, a.proof)
        print(cc.solidity_calldata(cc.read_proof_json(a.proof, device=dev, lib=lib), cc.read_public_json(a.public),
                                   device=dev, lib=lib))
        return 0
    if a.cmd == "wtns-check":
        _need(a.r1cs, a.wtns)
        r1cs = cc.R1CS.from_file(a.r1cs, lib=lib)
        w = cc.open_wtns(a.wtns, lib=lib)
        if w.n != r1cs.num_variables:
            raise ValueError(f"the witness has {w.n} values, the circuit {r1cs.num_variables} wires")
        row = cc.CircomBuilder(r1cs).build(w.to_montgomery(device=dev)).first_unsatisfied(lib=lib, device=dev)
        if row >= 0:
            print(f"INVALID: constraint {row} is not satisfied")
            return 1
        print("OK")
        return 0
    raise ValueError(f"unknown command {a.cmd}")


def main(argv=None, lib=None) -> int:
    """argv: the arguments after the program name (default sys.argv[1:]); lib: a _binding.Library (default: the
    product library).  Returns the exit status."""
    try:
        args = _parser().parse_args(argv)
    except SystemExit as e:   # argparse has printed its one usage line
        return int(e.code or 0)
    try:
        return _run(args, lib)
    except (cc.G16Error, OSError, ValueError, ImportError) as e:
        print(f"error: {e}", file=sys.stderr)
        return 2


if __name__ == "__main__":
    sys.exit(main())
