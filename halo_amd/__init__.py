"""halo_amd: MI355X (gfx950) backend for the rasmus-kirk/halo proving hot path.

The compute lives in libhalo_gpu.so (hand-written HIP behind the C ABI of include/halo_gpu.h);
this package is the thin host-side mirror of the reference's Rust surface on that path, with the
reference's names, argument meaning and assertion messages:

    halo_amd.group    -- crates/group/src/group.rs  (scalar_dot, point_dot_affine, construct_powers),
                         crates/group/src/pp.rs     (PublicParams: resident SRS)
    halo_amd.poly     -- crates/group/src/poly.rs   (Domain, Evals: NTT / iNTT wrappers)
    halo_amd.pedersen -- crates/accumulation/src/pedersen.rs (commit)
    halo_amd.pcdl     -- crates/accumulation/src/pcdl.rs     (commit, open_without_eval round loop,
                         succinct_check and check: the verifier's scalar multiplications as one batch)
    halo_amd.acc      -- crates/accumulation/src/acc.rs      (common_subroutine, prover, verifier, decider)
    halo_amd.schnorr  -- crates/schnorr/src/lib.rs (hash_message, PublicKey::verify) and the inner
                         Poseidon sponge of crates/poseidon, as batches of independent items
    halo_amd.plonk    -- crates/plonk/src/plonk/protocol.rs (PlonkProof, verify_succinct, verify: batches
                         of raw proofs of one circuit, every transcript on the device)
    halo_amd.sponge   -- crates/poseidon/src/outer_sponge.rs (Sponge: the Fiat-Shamir sponge as an object with
                         its state on the device; SpongeBatch: k of them in lockstep; new_transcript)
    halo_amd.wire     -- ark-serialize compressed bytes of Instance / EvalProof / Accumulator (pcdl.rs:26,159,
                         acc.rs:22) <-> the arrays above, decoded and encoded on the device

Field elements are numpy uint64 arrays of shape (n, 4) in arkworks Montgomery form; points are
(n, 8) WrappedPoint arrays (x, y Montgomery limbs; (0, 0) = identity).  There is no CPU fallback:
without the HIP library or a GPU every call raises.
"""
from . import _lib  # noqa: F401

__all__ = ["_lib", "group", "poly", "pedersen", "pcdl", "acc", "schnorr", "plonk", "sponge", "wire"]
