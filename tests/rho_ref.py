"""CPU restatement of the derived weights of the batched decider (halo_amd/csrc/decide_rho.hip behind
halo_pcdl_decide_rho; include/halo_gpu.h and DESIGN §4.9 state the derivation) over oracle/poseidon.py.
TEST INFRASTRUCTURE ONLY.  The derivation is this backend's own: the reference has no batched decider.

The batch is d, k, the live mask and the pairs (U_i, xi_{i,1..lg n}); xi_{i,0} is not hashed and nothing of an
instance that is not live is read.

  leaf_i   live: Sponge(BATCH_LEAF = 4).absorb_g(U_i).absorb_fr(xi_{i,1}) ... absorb_fr(xi_{i,lg n}), then the INNER
           sponge's squeeze(): a base-field element.  Not live: 0.
  tree     level l + 1 [j] = N(level l [2 j], level l [2 j + 1]) if 2 j + 1 < count else level l [2 j], until one
           element (the root) remains; N(a, b): a fresh unlabelled inner sponge absorbs a, b and squeezes once.
  seed     Sponge(BATCH_SEED = 5), its inner sponge absorbs root, k, d, squeezed once.
  rho_i    live: Sponge(BATCH_WEIGHT = 6), its inner sponge absorbs seed, i; challenge(), 0 replaced by 1.  Not live: 0.

Inputs and outputs are the arrays the library takes: xis (k, lg n + 1, 4) and rho (k, 4) ark scalars (Montgomery
limbs), Us (k, 8) WrappedPoints, (0, 0) the identity.  A coordinate is hashed as the field element its limbs denote.
"""
import numpy as np

import pasta as P
import poseidon

BATCH_LEAF, BATCH_SEED, BATCH_WEIGHT = 4, 5, 6


def _field(cname: str) -> str:
    return "fq" if cname == "pallas" else "fp"


def node(cname: str, a: int, b: int) -> int:
    s = poseidon.InnerSponge(_field(cname))
    s.absorb([a, b])
    return s.squeeze()


def leaf(cname: str, U, xi_row) -> int:
    """U: 8 limbs; xi_row: (lg n + 1, 4) limbs, row 0 not read."""
    cv = P.CURVES[cname]
    u = [int(w) for w in np.asarray(U).reshape(8)]
    s = poseidon.Sponge(cname, BATCH_LEAF)
    s.absorb_g([(P.from_mont(P.limbs_to_int(u[:4]), cv.base), P.from_mont(P.limbs_to_int(u[4:]), cv.base))])
    s.absorb_fr([P.from_mont(P.limbs_to_int(x), cv.scalar) for x in np.asarray(xi_row).reshape(-1, 4)[1:]])
    return s.inner.squeeze()


def root(cname: str, leaves) -> int:
    level = list(leaves)
    while len(level) > 1:
        level = [node(cname, level[j], level[j + 1]) if j + 1 < len(level) else level[j] for j in range(0, len(level), 2)]
    return level[0]


def zero_becomes_one(x: int) -> int:
    return x if x else 1


def weights_int(cname: str, xis, Us, d: int, live=None) -> list[int]:
    """The k weights as canonical integers."""
    U = np.asarray(Us, dtype=np.uint64).reshape(-1, 8)
    k = len(U)
    lg = (d + 1).bit_length() - 1
    x = np.asarray(xis, dtype=np.uint64).reshape(k, lg + 1, 4)
    on = [True] * k if live is None else [bool(b) for b in live]
    return weights_from_leaves(cname, [leaf(cname, U[i], x[i]) if on[i] else None for i in range(k)], d)


def weights_from_leaves(cname: str, leaves, d: int) -> list[int]:
    """... from the k leaves, None where the instance is not live (a test computes the leaves of its instances once
    and takes the weights of every prefix and mask from them)."""
    k = len(leaves)
    if k == 0:
        return []
    on = [x is not None for x in leaves]
    r = root(cname, [x if o else 0 for x, o in zip(leaves, on)])
    s = poseidon.Sponge(cname, BATCH_SEED)
    s.inner.absorb([r, k, d])
    seed = s.inner.squeeze()
    out = []
    for i in range(k):
        if not on[i]:
            out.append(0)
            continue
        w = poseidon.Sponge(cname, BATCH_WEIGHT)
        w.inner.absorb([seed, i])
        out.append(zero_becomes_one(w.challenge()))
    return out


def to_ark(cname: str, ws) -> np.ndarray:
    """canonical integers as (k, 4) ark scalars, what halo_pcdl_decide_rho writes"""
    m = P.CURVES[cname].scalar
    return np.array([P.int_to_limbs(P.to_mont(r, m)) for r in ws], dtype=np.uint64).reshape(-1, 4)


def weights(cname: str, xis, Us, d: int, live=None) -> np.ndarray:
    return to_ark(cname, weights_int(cname, xis, Us, d, live))
