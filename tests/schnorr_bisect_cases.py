"""Helpers of tests/test_gpu_schnorr_bisect.py: the pool of items that tests/test_gpu_schnorr_combined.py draws from
(tests/schnorr_combined_ref.signature_pool, six valid items and the special ones by name) with the restatement's
verdicts (tests/schnorr_ref.py), weights, resident buffers and the _dev call.  TEST INFRASTRUCTURE ONLY."""
import ctypes

import numpy as np

import pasta as P
import schnorr_combined_ref as CR
import schnorr_ref as SR

FULL = dict(schnorr_bisect_leaf=1, schnorr_bisect_pass_items=1)  # the full descent: no ladder, no budget
SCOPES = ("sig_t", "sig_scan_totals", "sig_node_scalars", "sig_split", "sig_bisect_msm", "sig_bisect_ladder")


class Items:
    """Distinct items (pk, msg, R, s), encoded once, with the restatement's verdicts; a batch is an index array."""

    def __init__(self, cname, msg_len, items):
        c = P.CURVES[cname]
        self.cname, self.msg_len, self.items = cname, msg_len, items
        self.pk = SR.points(cname, [it[0] for it in items])
        self.R = SR.points(cname, [it[2] for it in items])
        self.s = SR.fe_rows([it[3] for it in items], c.scalar)
        self.msgs = np.array([SR.fe_rows(it[1], c.base) for it in items], dtype=np.uint64).reshape(len(items), msg_len, 4)
        self.exp = np.array([SR.verify(cname, *it) for it in items], dtype=np.uint8)

    def take(self, idx):
        idx = np.asarray(idx)
        return (self.pk[idx], self.R[idx], self.s[idx], self.msgs[idx]), self.exp[idx]


CANCEL_X = 987654321


def variants(cname, msg_len=10):
    """The pool's six valid items, then the special ones by name -> (Items, {name: index})."""
    c = P.CURVES[cname]
    sks, pool = CR.signature_pool(cname, msg_len)
    pk, msg, R, s = pool[0]
    other = pool[1]
    named = {
        "s_plus_1": (pk, msg, R, (s + 1) % c.scalar),
        "altered_msg": (pk, msg[:-1] + ((msg[-1] + 1) % c.base,), R, s),
        "other_pk": (other[0], msg, R, s),
        "other_R": (pk, msg, other[2], s),
        "pk_off_curve": (((pk[0] + 1) % c.base, pk[1]), msg, R, s),
        "R_off_curve": (pk, msg, (R[0], (R[1] + 1) % c.base), s),
        "dead_and_wrong": (((pk[0] + 1) % c.base, pk[1]), msg, R, (s + 1) % c.scalar),
        # errors that cancel under equal weights: item 0 with s + x, item 1 with s - x
        "plus_x": (pk, msg, R, (s + CANCEL_X) % c.scalar),
        "minus_x": (other[0], other[1], other[2], (other[3] - CANCEL_X) % c.scalar),
    }
    R0, s0 = SR.sign(cname, 0, 777, msg)  # sk = 0: pk = identity, s = the nonce
    named["pk_identity"] = (None, msg, R0, s0)
    Rn, sn = SR.sign(cname, sks[1], 0, msg)  # nonce 0: R = identity, s = e sk
    named["R_identity"] = (SR.public_key(cname, sks[1]), msg, Rn, sn)
    Rp, sp = SR.sign(cname, sks[2], sks[2], msg)  # nonce = sk: R = pk
    named["R_equals_pk"] = (SR.public_key(cname, sks[2]), msg, Rp, sp)
    names = list(named)
    return Items(cname, msg_len, pool + [named[n] for n in names]), {n: len(pool) + j for j, n in enumerate(names)}


def rand_rho(k, seed):
    """k uniform ark scalars below 2^254, so below either modulus; nonzero but for a chance of 2^-254."""
    a = np.random.default_rng(seed).integers(0, 1 << 64, size=(k, 4), dtype=np.uint64)
    a[:, 3] >>= np.uint64(2)
    return a


def small_rho(cname, ws):
    return SR.fe_rows(ws, P.CURVES[cname].scalar)


def cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def dev(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


def bisect_dev(hal, cname, arrs, rho, stream=None):
    """halo_schnorr_verify_bisect_dev over resident inputs -> (ok bytes, combined byte); rho None: derived."""
    import torch
    pk, R, s, msgs = arrs
    k, msg_len = len(pk), msgs.shape[1]
    d = [cuda(x) for x in (pk, R, s, msgs)]
    d_rho = cuda(rho) if rho is not None else None
    d_ok = torch.full((k,), 7, dtype=torch.uint8, device="cuda")
    d_comb = torch.full((1,), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    st = stream or torch.cuda.current_stream()
    hal.check(hal.load().halo_schnorr_verify_bisect_dev(hal.CURVES[cname], *[dev(t) for t in d], msg_len, k, dev(d_rho),
                                                        dev(d_ok), dev(d_comb), ctypes.c_void_p(st.cuda_stream)))
    st.synchronize()
    return d_ok.cpu().numpy(), int(d_comb.cpu()[0])


class Launches:
    """``with Launches(hal) as n: ...; n()`` -> {scope: launches} of the descent's profile scopes inside the block."""

    def __init__(self, hal):
        self.hal, self.L = hal, hal.load()

    def __enter__(self):
        self.hal.check(self.L.halo_profile_reset())
        self.hal.check(self.L.halo_profile_enable(1))
        return self

    def __call__(self):
        out = {}
        for name in SCOPES:
            cnt, ms = ctypes.c_size_t(0), ctypes.c_double(0.0)
            self.hal.check(self.L.halo_profile_read(name.encode(), ctypes.byref(cnt), ctypes.byref(ms)))
            out[name] = cnt.value
        return out

    def __exit__(self, *exc):
        self.hal.check(self.L.halo_profile_enable(0))
        self.hal.check(self.L.halo_profile_reset())
        return False
