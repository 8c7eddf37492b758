//! Batch verification on the GPU: `Groth16::<Bn254>::process_vk` + `verify_with_processed_vk`
//! (reference call sites src/zkey.rs:868-870,914-916) for many proofs under one key:
//! `verify_batch` (`g16_verify_batch`, one GPU lane and one full pairing check per proof) and
//! `verify_aggregate` (`g16_verify_aggregate`, ONE combined check for the whole batch).  The CPU
//! call keeps working unchanged; these are for batches.
use ark_bn254::{Bn254, Fr};
use ark_groth16::{Proof, VerifyingKey};

use crate::ffi;
use crate::pack;
use crate::prover::GpuError;

/// The packed forms the C ABI takes; `ic` backs the pointer inside `desc`.
struct Packed {
    desc: ffi::g16_vk_desc,
    _ic: Vec<u8>,
    raw: Vec<u8>,
    pubs: Vec<u64>,
}

fn pack_batch(vk: &VerifyingKey<Bn254>, public_inputs: &[Vec<Fr>], proofs: &[Proof<Bn254>]) -> Result<Packed, GpuError> {
    let n = proofs.len();
    let n_pub = vk.gamma_abc_g1.len() - 1;
    if public_inputs.len() != n || public_inputs.iter().any(|p| p.len() != n_pub) {
        // SynthesisError::MalformedVerifyingKey in ark-groth16's prepare_inputs
        return Err(GpuError::Synthesis(ark_relations::r1cs::SynthesisError::MalformedVerifyingKey));
    }
    let ic = pack::pack_g1_vec(&vk.gamma_abc_g1);
    let mut desc = ffi::g16_vk_desc {
        alpha_g1: [0; 64],
        beta_g2: [0; 128],
        gamma_g2: [0; 128],
        delta_g2: [0; 128],
        ic: ic.as_ptr(),
        ic_count: vk.gamma_abc_g1.len() as u32,
    };
    pack::pack_g1(&vk.alpha_g1, &mut desc.alpha_g1);
    pack::pack_g2(&vk.beta_g2, &mut desc.beta_g2);
    pack::pack_g2(&vk.gamma_g2, &mut desc.gamma_g2);
    pack::pack_g2(&vk.delta_g2, &mut desc.delta_g2);
    let mut raw = vec![0u8; ffi::G16_PROOF_BYTES * n];
    for (p, o) in proofs.iter().zip(raw.chunks_exact_mut(ffi::G16_PROOF_BYTES)) {
        pack::pack_g1(&p.a, &mut o[0..64]);
        pack::pack_g2(&p.b, &mut o[64..192]);
        pack::pack_g1(&p.c, &mut o[192..256]);
    }
    let mut pubs: Vec<u64> = Vec::with_capacity(4 * n * n_pub);
    for v in public_inputs {
        pubs.extend_from_slice(&pack::fr_vec_words(v));
    }
    Ok(Packed { desc, _ic: ic, raw, pubs })
}

/// `out[i]` = `verify_with_processed_vk(&process_vk(vk), &public_inputs[i], &proofs[i])`
pub fn verify_batch(
    vk: &VerifyingKey<Bn254>,
    public_inputs: &[Vec<Fr>],
    proofs: &[Proof<Bn254>],
    device: i32,
) -> Result<Vec<bool>, GpuError> {
    let n = proofs.len();
    let p = pack_batch(vk, public_inputs, proofs)?;
    let mut ok = vec![0u8; n];
    let st = unsafe { ffi::g16_verify_batch(device, &p.desc, p.raw.as_ptr(), p.pubs.as_ptr(), n as u32, ok.as_mut_ptr()) };
    if st != ffi::G16_OK {
        return Err(GpuError::Library(st, "g16_verify_batch failed".into()));
    }
    Ok(ok.into_iter().map(|b| b != 0).collect())
}

/// All proofs in ONE combined pairing check (the small-exponent batch test): `true` iff every
/// `verify_with_processed_vk(.., &public_inputs[i], &proofs[i])` is, up to a soundness error of
/// 2^-127.  `rho`: `None` (the library draws 128-bit coefficients from the operating system's
/// CSPRNG) or one non-zero coefficient per proof -- derived from a transcript hash that covers the
/// proofs, never known to whoever made them: a prover who knows `rho` can forge a passing batch of
/// invalid proofs.
pub fn verify_aggregate(
    vk: &VerifyingKey<Bn254>,
    public_inputs: &[Vec<Fr>],
    proofs: &[Proof<Bn254>],
    rho: Option<&[u128]>,
    device: i32,
) -> Result<bool, GpuError> {
    let n = proofs.len();
    let p = pack_batch(vk, public_inputs, proofs)?;
    let words: Option<Vec<u64>> = match rho {
        Some(r) if r.len() != n => return Err(GpuError::Library(ffi::G16_ERR_INVALID, "one coefficient per proof".into())),
        Some(r) => Some(r.iter().flat_map(|x| [*x as u64, (*x >> 64) as u64]).collect()),
        None => None,
    };
    let rho_ptr = words.as_ref().map_or(std::ptr::null(), |w| w.as_ptr());
    let mut ok = 0u8;
    let st = unsafe {
        ffi::g16_verify_aggregate(device, &p.desc, p.raw.as_ptr(), p.pubs.as_ptr(), n as u32, rho_ptr, &mut ok, std::ptr::null_mut())
    };
    if st != ffi::G16_OK {
        return Err(GpuError::Library(st, "g16_verify_aggregate failed".into()));
    }
    Ok(ok != 0)
}

/// One group of `verify_aggregate_keys`: a key with the proofs under it and their public inputs.
pub type KeyGroup<'a> = (&'a VerifyingKey<Bn254>, &'a [Vec<Fr>], &'a [Proof<Bn254>]);

/// Proofs under MANY keys in one pass (`g16_verify_aggregate_keys`): `out[k]` is what
/// `verify_aggregate(groups[k].0, groups[k].1, groups[k].2, rho[k], device)` returns -- the combined
/// check over group k alone, nothing is summed across groups -- for about the cost of one such call,
/// whatever the number of keys.  `rho`: `None` (drawn by the library) or one slice per group, under
/// the rules of `verify_aggregate`.
pub fn verify_aggregate_keys(groups: &[KeyGroup], rho: Option<&[&[u128]]>, device: i32) -> Result<Vec<bool>, GpuError> {
    if let Some(r) = rho {
        if r.len() != groups.len() || r.iter().zip(groups).any(|(r, g)| r.len() != g.2.len()) {
            return Err(GpuError::Library(ffi::G16_ERR_INVALID, "one coefficient per proof".into()));
        }
    }
    let packed: Vec<Packed> = groups.iter().map(|(vk, inputs, proofs)| pack_batch(vk, inputs, proofs)).collect::<Result<_, _>>()?;
    let descs: Vec<*const ffi::g16_vk_desc> = packed.iter().map(|p| &p.desc as *const _).collect();
    let counts: Vec<u32> = groups.iter().map(|g| g.2.len() as u32).collect();
    let raw: Vec<u8> = packed.iter().flat_map(|p| p.raw.iter().copied()).collect();
    let pubs: Vec<u64> = packed.iter().flat_map(|p| p.pubs.iter().copied()).collect();
    let words: Option<Vec<u64>> = rho.map(|r| r.iter().flat_map(|g| g.iter().flat_map(|x| [*x as u64, (*x >> 64) as u64])).collect());
    let rho_ptr = words.as_ref().map_or(std::ptr::null(), |w| w.as_ptr());
    let mut ok = vec![0u8; groups.len()];
    let st = unsafe {
        ffi::g16_verify_aggregate_keys(device, descs.as_ptr(), counts.as_ptr(), groups.len() as u32, raw.as_ptr(), pubs.as_ptr(), rho_ptr, ok.as_mut_ptr(), std::ptr::null_mut())
    };
    if st != ffi::G16_OK {
        return Err(GpuError::Library(st, "g16_verify_aggregate_keys failed".into()));
    }
    Ok(ok.into_iter().map(|b| b != 0).collect())
}

/// `Groth16::<Bn254>::rerandomize_proof(vk, proof, rng)` for a batch under one key on the GPU
/// (`g16_proofs_rerandomize`), one lane per proof:
/// `A' = r1^-1 A`, `B' = r1 B + (r1 r2) delta`, `C' = C + r2 A`.  `scalars`: `None` (the library draws every
/// `(r1, r2)` from the operating system's CSPRNG and wipes them) or one `(r1, r2)` per proof with `r1 != 0`.
/// Nothing is verified: the new proof is valid exactly when the old one was.
pub fn rerandomize_proofs(
    vk: &VerifyingKey<Bn254>,
    proofs: &[Proof<Bn254>],
    scalars: Option<&[(Fr, Fr)]>,
    device: i32,
) -> Result<Vec<Proof<Bn254>>, GpuError> {
    let n = proofs.len();
    let words: Option<Vec<u64>> = match scalars {
        Some(s) if s.len() != n => return Err(GpuError::Library(ffi::G16_ERR_INVALID, "one (r1, r2) per proof".into())),
        Some(s) => Some(s.iter().flat_map(|(r1, r2)| pack::fr_words(r1).into_iter().chain(pack::fr_words(r2))).collect()),
        None => None,
    };
    let mut delta = [0u8; 128];
    pack::pack_g2(&vk.delta_g2, &mut delta);
    let mut raw = vec![0u8; ffi::G16_PROOF_BYTES * n];
    for (p, o) in proofs.iter().zip(raw.chunks_exact_mut(ffi::G16_PROOF_BYTES)) {
        pack::pack_g1(&p.a, &mut o[0..64]);
        pack::pack_g2(&p.b, &mut o[64..192]);
        pack::pack_g1(&p.c, &mut o[192..256]);
    }
    let sc_ptr = words.as_ref().map_or(std::ptr::null(), |w| w.as_ptr());
    // in place: proofs_out == proofs is supported
    let st = unsafe {
        ffi::g16_proofs_rerandomize(device, delta.as_ptr(), raw.as_ptr(), n as u32, sc_ptr, raw.as_mut_ptr(), std::ptr::null_mut())
    };
    if st != ffi::G16_OK {
        return Err(GpuError::Library(st, "g16_proofs_rerandomize failed".into()));
    }
    Ok(raw
        .chunks_exact(ffi::G16_PROOF_BYTES)
        .map(|c| {
            let rec: &[u8; 256] = c.try_into().expect("256-byte record");
            pack::unpack_proof(rec)
        })
        .collect())
}

/// `PreparedVerifyingKey<Bn254>` on the device (`g16_pvk`): what `Groth16Gpu::process_vk` returns.  The key has
/// been tested (canonical coordinates, points on their curves, G2 points in the subgroup); the handle holds the
/// Miller value of (beta, -alpha) and the line tables of gamma and delta.  Dropping it releases the device memory.
pub struct GpuPreparedVerifyingKey {
    ptr: *mut ffi::g16_pvk,
    n_pub: usize,
}

// calls on one handle serialise on a mutex inside the library
unsafe impl Send for GpuPreparedVerifyingKey {}
unsafe impl Sync for GpuPreparedVerifyingKey {}

impl Drop for GpuPreparedVerifyingKey {
    fn drop(&mut self) {
        unsafe { ffi::g16_pvk_destroy(self.ptr) }
    }
}

/// `Groth16::<Bn254>::process_vk(vk)` on the GPU (`g16_pvk_create`)
pub fn process_vk(vk: &VerifyingKey<Bn254>, device: i32) -> Result<GpuPreparedVerifyingKey, GpuError> {
    let p = pack_batch(vk, &[], &[])?;
    let mut ptr: *mut ffi::g16_pvk = std::ptr::null_mut();
    let st = unsafe { ffi::g16_pvk_create(device, &p.desc, &mut ptr) };
    if st != ffi::G16_OK {
        let msg = unsafe { std::ffi::CStr::from_ptr(ffi::g16_last_error(std::ptr::null())) }.to_string_lossy().into_owned();
        return Err(GpuError::Library(st, msg));
    }
    Ok(GpuPreparedVerifyingKey { ptr, n_pub: vk.gamma_abc_g1.len() - 1 })
}

/// `out[i]` = `verify_with_processed_vk(pvk, &public_inputs[i], &proofs[i])` (`g16_verify_prepared`): one
/// workgroup per proof, the low-latency form; the verdicts are `verify_batch`'s.
pub fn verify_prepared(
    pvk: &GpuPreparedVerifyingKey,
    public_inputs: &[Vec<Fr>],
    proofs: &[Proof<Bn254>],
) -> Result<Vec<bool>, GpuError> {
    let n = proofs.len();
    if public_inputs.len() != n || public_inputs.iter().any(|p| p.len() != pvk.n_pub) {
        return Err(GpuError::Synthesis(ark_relations::r1cs::SynthesisError::MalformedVerifyingKey));
    }
    let mut raw = vec![0u8; ffi::G16_PROOF_BYTES * n];
    for (p, o) in proofs.iter().zip(raw.chunks_exact_mut(ffi::G16_PROOF_BYTES)) {
        pack::pack_g1(&p.a, &mut o[0..64]);
        pack::pack_g2(&p.b, &mut o[64..192]);
        pack::pack_g1(&p.c, &mut o[192..256]);
    }
    let mut pubs: Vec<u64> = Vec::with_capacity(4 * n * pvk.n_pub);
    for v in public_inputs {
        pubs.extend_from_slice(&pack::fr_vec_words(v));
    }
    let mut ok = vec![0u8; n];
    let st = unsafe { ffi::g16_verify_prepared(pvk.ptr, raw.as_ptr(), pubs.as_ptr(), n as u32, ok.as_mut_ptr()) };
    if st != ffi::G16_OK {
        return Err(GpuError::Library(st, "g16_verify_prepared failed".into()));
    }
    Ok(ok.into_iter().map(|b| b != 0).collect())
}

impl crate::Groth16Gpu {
    /// `Groth16::<Bn254>::process_vk(&vk)` on the GPU: the key is tested, its (beta, -alpha) Miller value and
    /// the line tables of gamma and delta are built once and stay on the device.
    pub fn process_vk(vk: &VerifyingKey<Bn254>, device: i32) -> Result<GpuPreparedVerifyingKey, GpuError> {
        process_vk(vk, device)
    }

    /// `Groth16::<Bn254>::verify_with_processed_vk(&pvk, public_inputs, &proof)` on the GPU: one workgroup
    /// checks the proof (a few milliseconds, not the some hundred of the one-lane-per-proof verifiers).
    pub fn verify_with_processed_vk(
        pvk: &GpuPreparedVerifyingKey,
        public_inputs: &[Fr],
        proof: &Proof<Bn254>,
    ) -> Result<bool, GpuError> {
        Ok(verify_prepared(pvk, &[public_inputs.to_vec()], std::slice::from_ref(proof))?[0])
    }
}
