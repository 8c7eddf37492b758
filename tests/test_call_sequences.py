"""Call sequences on ONE ctx: changing witnesses, changing (r, s), every entry point.

The parity tests compare one call on a fresh ctx.  A g16_ctx carries state from call to call -- four streams and
their events, staging buffers shared by unrelated entry points (w_dev, h_dev, sums_dev, out_dev, rs_dev), the
fix list and its overflow flag, the entry count of the last sort, the filtered B view, the batch workspace and its
capacity, the lazily allocated ingest words, the cached (r, s) of the sharded finish, the profiling switch -- and a
missing ordering edge or a stale count shows only when the NEXT call brings other data.  So here:

  * neighbouring steps never share a witness, an (r, s) pair or a scalar vector (`Session._fresh` enforces it;
    the one exception is the hit path of the sharded finish, which needs the same (r, s) twice);
  * the witness pool differs in SIZE of derived state as well as in value: satisfying witnesses, dense random
    vectors, vectors of mostly 0 / 1 / r - 1, all zeros with w[0] = 1 (almost no sort entries: whatever is read
    beyond the new entry count is the previous call's) and all r - 1;
  * every output of every step is compared with a value computed outside the library under test: the C
    restatement (cpu_ref.prove / msm_g1 / msm_g2 / witness_map, pinned to bn254_ref by tests/test_oracle.py),
    computed once per (configuration, witness id, (r, s) id) and cached for the module;
  * in every sequence one proof of a satisfying witness is pairing-verified by bn254_ref and rejected for a wrong
    public input.

Configurations (the smallest key that reaches the branch; Prover.info() is asserted):
  T   fixed-base tables (automatic rule)            B   bucket path, default overlap schedule
  R   window_bits = 19, large-bucket-set schedule   S   G16_SPARSE_B=1, most B points at infinity
  W2  world = 2, both cuts                          M   devices = [0, 0]
  WM  witness-map-only ctx                          F   a key of equal points: the fix list is used by every launch

The scripted sequences run on the emulator and on the GPU; the seeded walks (a pure function of (config, seed):
the assertion message carries config, seed, step and the operation names so far, so that a failure can be
replayed as a scripted sequence) and the two-thread sibling test run on the GPU only."""
import os
import random
import threading

import numpy as np
import pytest

import bn254_ref as o
import helpers as H

R = o.R_MOD
G16_ERR_INVALID = 1
NW, NRS = 12, 10          # witnesses / (r, s) pairs per configuration
SAT = (0, 1, 2)           # pool indices of the satisfying witnesses
QUERY_A, QUERY_B1, QUERY_L, QUERY_H, QUERY_B2 = 0, 1, 2, 3, 4


def _is_emu(lib):
    return lib.path.endswith("libg16_emu.so")


def _le(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype=np.uint8).reshape(-1, 32).copy()


# ---- circuits ----------------------------------------------------------------------------------------------------
def _chain(k):
    cons, _, n_vars, n_pub = H.squaring_chain(k)
    return cons, n_vars, n_pub, [H.squaring_chain(k, x0=x0)[1] for x0 in (3, 5, 2 ** 200 + 7)]


def _sparse_b(n_rows):
    """the shape of test_kernels' sparse-B circuit: four fresh wires per row, one row in four with a B wire of its
    own -- every other wire has the point at infinity in both B queries.  Three satisfying witnesses."""
    def build(seed):
        rng = random.Random(seed)
        w, cons = [1, 0], []
        for i in range(n_rows):
            a, b = rng.randrange(R), rng.choice([0, 1, 1, rng.randrange(R)])
            base = len(w)
            w.extend([a, rng.randrange(2), rng.randrange(R), 0])
            if i % 4 == 0:
                w[base + 1] = b
                cons.append(([(base, 1), (base + 2, 3)], [(base + 1, 1)], [(base + 3, 1)]))
                w[base + 3] = (a + 3 * w[base + 2]) * b % R
            else:
                cons.append(([(base, 1), (base + 1, 2)], [(0, 1)], [(base + 3, 1)]))
                w[base + 3] = (a + 2 * w[base + 1]) % R
        cons.append(([(len(w) - 1, 1)], [(0, 1)], [(1, 1)]))
        w[1] = w[-1]
        return cons, w
    cons, w0 = build(11)
    sat = [w0, build(12)[1], build(13)[1]]
    assert all(build(s)[0] == cons for s in (12, 13))
    return cons, len(w0), 1, sat


def _same_point_key(n):
    """the key of test_optimistic_accumulation_overflow_...: every point of A, B1, L and H is ONE point, so every
    mixed addition after a lane's first meets equal x-coordinates and the optimistic G1 kernel sets it aside in
    the fix list -- here few enough (25 segments of 8 entries defer 7 each) that the list does NOT overflow and
    k_acc_fixup adds them.  Not a key of any circuit: bytes are compared, nothing is pairing-verified."""
    rng = random.Random(812)
    N = n + 1
    P, Q = o.G1.mul(o.G1_GEN, 12345), o.G2.mul(o.G2_GEN, 54321)
    base, g2 = H.rand_g1(rng, 3), H.rand_g2(rng, 3)
    pk = dict(n_vars=N, n_public=1, domain_size=4, alpha_g1=base[0], beta_g1=base[1], beta_g2=g2[0], gamma_g2=g2[1],
              delta_g1=base[2], delta_g2=g2[2], ic=base[:2], a_query=[P] * N, b_g1_query=[P] * N,
              b_g2_query=[Q] * N, l_query=[P] * (N - 2), h_query=[P] * 4)
    ones = [1] * N
    few = [1] * N
    for i in range(3, N, 17):
        few[i] = rng.randrange(R)
    return dict(pk=pk, cons=[([(1, 1)], [(0, 1)], [])], n_vars=N, n_pub=1, first=[ones, [1] + [2] * n, few])


# id -> (circuit on the emulator, circuit on the GPU, Prover options); None: not run there (window_bits = 19 takes
# the emulator two minutes per three proofs; test_reduce_tail_split steps through that path once)
CONFIGS = {
    "T": (lambda: _chain(4), lambda: _chain(6), dict(tables=0)),
    "B": (lambda: _chain(5), lambda: _chain(10), dict(tables=-1)),
    "R": (None, lambda: _chain(12), dict(tables=-1, window_bits=19)),
    "S": (lambda: _sparse_b(15), lambda: _sparse_b(375), dict(tables=-1)),
    "W2": (lambda: _chain(4), lambda: _chain(5), dict(tables=-1)),
    "M": (lambda: _chain(4), lambda: _chain(5), dict(tables=-1, devices=[0, 0])),
    "WM": (lambda: _chain(4), lambda: _chain(10), dict()),
    "F": (lambda: _same_point_key(200), lambda: _same_point_key(200), dict(tables=-1, window_bits=16)),
}


class Config:
    """circuit, key, pools and the cached expected values of one configuration on one library"""

    def __init__(self, name, lib):
        import circom_compat_amd as cc
        emu = _is_emu(lib)
        make = CONFIGS[name][0 if emu else 1]
        self.name, self.lib, self.cc, self.emu = name, lib, cc, emu
        self.opts = dict(CONFIGS[name][2])
        if name == "B" and emu:     # as test_msm_hot_bucket_split: the plane precomputation stays cheap
            self.opts.update(window_bits=5, planes=3)
        made = make()
        raw = made["pk"] if isinstance(made, dict) else None      # config F: a key given point by point
        cons, self.n_vars, self.n_pub, sat = ((made["cons"], made["n_vars"], made["n_pub"], made["first"]) if raw
                                              else made)
        self.m = len(cons)
        rng = random.Random("call-sequences " + name)
        rows = lambda k: [[(wdx, c) for wdx, c in con[k]] for con in cons]

        def csr(k):      # coefficients through the oracle's Montgomery conversion, not the library's
            rp, col, val = [0], [], []
            for row in rows(k):
                col += [wdx for wdx, _ in row]
                val += [c for _, c in row]
                rp.append(len(col))
            return cc.Csr(rp, col, H.fr_mont_arr(val))
        a, b, c = csr(0), csr(1), csr(2)
        self.mats = cc.ConstraintMatrices(self.n_pub + 1, self.n_vars - self.n_pub, self.m, a, b)
        self.pk = H.pk_from_oracle(raw) if raw else cc.trapdoor_setup(
            a, b, c, self.n_vars, self.n_pub, [rng.randrange(1, R) for _ in range(5)], lib=lib)
        self.domain = self.pk.domain_size
        pk = self.pk
        self.vk = dict(alpha_g1=o.g1_from_bytes(bytes(pk.vk.alpha_g1)), beta_g2=o.g2_from_bytes(bytes(pk.vk.beta_g2)),
                       gamma_g2=o.g2_from_bytes(bytes(pk.vk.gamma_g2)), delta_g2=o.g2_from_bytes(bytes(pk.vk.delta_g2)),
                       ic=[o.g1_from_bytes(bytes(x)) for x in pk.vk.gamma_abc_g1])
        n = self.n_vars

        def dense():
            return [1] + [rng.randrange(R) for _ in range(n - 1)]

        def skewed():
            return [1] + [rng.choice([0, 1, 1, R - 1]) if rng.random() < 0.9 else rng.randrange(R) for _ in range(n - 1)]
        self.w_ints = [sat[0], sat[1], sat[2], dense(), skewed(), [1] + [0] * (n - 1), dense(), [R - 1] * n,
                       skewed(), dense(), skewed(), dense()]
        self.w_names = ["sat0", "sat1", "sat2", "dense0", "skewed0", "zeros", "dense1", "all-r-1", "skewed1", "dense2",
                        "skewed2", "dense3"]
        assert len(self.w_ints) == NW and all(len(w) == n for w in self.w_ints)
        self.w_mont = [H.fr_mont_arr(w) for w in self.w_ints]
        self.w_le = [_le(w) for w in self.w_ints]
        self.rs_ints = [(0, 0)] + [(rng.randrange(R), rng.randrange(R)) for _ in range(NRS - 3)] + [(R - 1, 1), (0, 7)]
        assert len(self.rs_ints) == NRS
        self.rs_mont = [H.fr_mont_arr(list(p)) for p in self.rs_ints]
        # the (witness, (r, s)) combinations the sequences draw from: two per witness, dealt so that neighbours
        # (and any five in a row: one batch) differ in both
        self.combos = [(wi, wi % NRS) for wi in range(NW)] + [(wi, (wi + 3) % NRS) for wi in range(NW)]
        # scalar vectors per query: id -> ints; lengths from 1 to the whole query
        full = n - 1
        self.scalars = {
            QUERY_A: [dense()[1:], [rng.randrange(R)], skewed()[1:], dense()[1:full // 2 + 1]],
            QUERY_B1: [dense()[1:], skewed()[1:], [rng.randrange(R), 1]],
            QUERY_B2: [dense()[1:], [rng.randrange(R)], [R - 1, rng.randrange(R)], skewed()[1:]],
            QUERY_L: [dense()[1:full - self.n_pub + 1], skewed()[1:full - self.n_pub + 1], [rng.randrange(R)]],
            QUERY_H: [[rng.randrange(R) for _ in range(self.domain)], [rng.randrange(R) for _ in range(self.domain)],
                      [rng.randrange(R) for _ in range(3)]],
        }
        self.bases = {QUERY_A: pk.a_query[1:], QUERY_B1: pk.b_g1_query[1:], QUERY_B2: pk.b_g2_query[1:],
                      QUERY_L: pk.l_query, QUERY_H: pk.h_query}
        self._proofs, self._h, self._msm, self._verified = {}, {}, {}, {}

    # -- expected values: the C restatement, once per id
    def want_proof(self, wi, ri):
        if (wi, ri) not in self._proofs:
            import cpu_ref
            rs = self.rs_mont[ri]
            self._proofs[wi, ri] = cpu_ref.prove(self.pk, self.mats, rs[0:1].copy(), rs[1:2].copy(), self.w_mont[wi])
        return self._proofs[wi, ri]

    def want_h(self, wi):
        if wi not in self._h:
            import cpu_ref
            self._h[wi] = cpu_ref.witness_map(self.mats.a, self.mats.b, self.n_pub + 1, self.m, self.w_mont[wi])
        return self._h[wi]

    def want_msm(self, q, si):
        if (q, si) not in self._msm:
            import cpu_ref
            sc = H.fr_mont_arr(self.scalars[q][si])
            bases = np.ascontiguousarray(self.bases[q][:len(sc)])
            self._msm[q, si] = (cpu_ref.msm_g2 if q == QUERY_B2 else cpu_ref.msm_g1)(bases, sc)
        return self._msm[q, si]

    def verify(self, wi, raw):
        """pairing check by the oracle, once per distinct proof; a wrong public input is rejected"""
        assert wi in SAT and self.name != "F"
        if raw not in self._verified:
            pub = self.w_ints[wi][1:1 + self.n_pub]
            proof = H.proof_from_bytes(raw)
            self._verified[raw] = (o.verify_proof(self.vk, pub, proof)
                                   and not o.verify_proof(self.vk, [(pub[0] + 1) % R] + pub[1:], proof))
        return self._verified[raw]

    def prover(self, **kw):
        opts = dict(self.opts, **kw)
        env = os.environ.get("G16_SPARSE_B")
        if self.name == "S":
            os.environ["G16_SPARSE_B"] = "1"     # read when the ctx is created
        try:
            if self.name == "WM":
                pr = self.cc.Prover(None, self.mats, lib=self.lib, n_vars=self.n_vars, **opts)
            else:
                pr = self.cc.Prover(self.pk, self.mats, lib=self.lib, **opts)
        finally:
            if self.name == "S":
                if env is None:
                    del os.environ["G16_SPARSE_B"]
                else:
                    os.environ["G16_SPARSE_B"] = env
        info = pr.info()
        if self.name == "T":
            assert info["fixed_tables"] == 1
        elif self.name != "WM":
            assert info["fixed_tables"] == 0
        if self.name == "R":
            assert info["c_w"] == 19                 # 2^18 buckets: the large-bucket-set branch
        if self.name == "B" and self.emu:
            assert info["c_w"] == 5 and info["planes_w"] == 3
        if self.name == "S":
            n_inf = int((~self.pk.b_g1_query[1:].any(axis=1)).sum())
            assert info["sparse_b"] == 1 and 3 * n_inf >= self.n_vars
        if self.name == "M":
            assert info["devices"] == 2
        return pr


_configs = {}


def config(name, lib):
    key = (name, lib.path)
    if key not in _configs:
        _configs[key] = Config(name, lib)
    return _configs[key]


class Deal:
    """deals Config.combos in order from `start`: neighbours differ in witness and in (r, s)"""

    def __init__(self, cfg, start=0):
        self.cfg, self.i = cfg, start

    def __call__(self, k=None):
        out = [self.cfg.combos[(self.i + j) % len(self.cfg.combos)] for j in range(k or 1)]
        self.i += k or 1
        return out if k else out[0]


_donors = {}


class Session:
    """one ctx and the checked form of every call on it.  Each method performs the call, compares its output with
    the expected value and records its name; `_fresh` refuses a step that shares a witness, an (r, s) or a scalar
    vector with the step before it."""

    def __init__(self, cfg, label="", **kw):
        self.cfg, self.label = cfg, label
        if cfg.name == "T" and cfg.emu:
            # the emulator needs 45 s for the tables of these 16 wires: there every T ctx is a sibling of one donor
            # that lends them -- a ctx of its own in everything this module is about (streams, events, staging
            # buffers, batch workspace); on the GPU every sequence has a ctx created from the key
            if cfg.lib.path not in _donors:
                _donors[cfg.lib.path] = cfg.prover()
            kw = dict(kw, sibling_of=_donors[cfg.lib.path])
        self.pr = cfg.prover(**kw)
        self.ops = []
        self.last = dict(w=set(), rs=set(), sc=set())
        self.resident = None           # pool index of the witness g16_witness_buffer holds
        self.proofs = []               # (wi, raw) of every proof returned
        self.keep = []                 # the caller's own device buffers
        self.multi = "devices" in cfg.opts

    def close(self):
        self.keep.clear()
        self.pr.close()

    def _ctx(self):
        return f"config {self.cfg.name} {self.label} step {len(self.ops) - 1}: {' > '.join(self.ops)}"

    def _fresh(self, op, w=(), rs=(), sc=()):
        self.ops.append(op)
        now = dict(w=set(w), rs=set(rs), sc=set(sc))
        for k in now:
            assert not (now[k] & self.last[k]), f"sequence error: neighbouring steps share {k} {now[k] & self.last[k]}: " + self._ctx()
            if now[k]:
                self.last[k] = now[k]

    def _proof(self, wi, ri, raw):
        assert raw == self.cfg.want_proof(wi, ri), \
            f"proof of witness {self.cfg.w_names[wi]} with (r, s) #{ri} differs from the CPU restatement: " + self._ctx()
        self.proofs.append((wi, raw))

    def _refused(self, fn, *a):
        with pytest.raises(self.cfg.cc.G16Error) as e:
            fn(*a)
        assert e.value.status == G16_ERR_INVALID, self._ctx()
        return e.value

    # -- witnesses from the host
    def prove(self, wi, ri):
        self._fresh("prove", [wi], [ri])
        self.resident = None
        self._proof(wi, ri, self.pr.prove(*self.cfg.rs_ints[ri], self.cfg.w_mont[wi]).raw)

    def prove_wtns(self, wi, ri):
        self._fresh("prove_wtns", [wi], [ri])
        self.resident = None
        self._proof(wi, ri, self.pr.prove_wtns(self.cfg.w_le[wi], *self.cfg.rs_ints[ri]).raw)

    def prove_wtns_refused(self, wi, ri, element=None):
        """one element >= r: G16_ERR_INVALID naming it, no proof"""
        self._fresh("prove_wtns_refused", [wi], [ri])
        self.resident = None
        e = self.cfg.n_vars - 2 if element is None else element
        bad = self.cfg.w_le[wi].copy()
        bad[e] = np.frombuffer(R.to_bytes(32, "little"), dtype=np.uint8)
        err = self._refused(self.pr.prove_wtns, bad, *self.cfg.rs_ints[ri])
        assert f"element {e}" in str(err), self._ctx()

    def upload(self, wi, canonical=False):
        self._fresh("upload_witness_canonical" if canonical else "upload_witness", [wi])
        self.resident = None
        ptr = (self.pr.upload_witness_canonical(self.cfg.w_le[wi]) if canonical
               else self.pr.upload_witness(self.cfg.w_mont[wi]))
        assert ptr and ptr == self.pr.witness_buffer(), self._ctx()
        self.resident = wi

    # -- witnesses on the device
    def prove_resident(self, ri):
        assert self.resident is not None, "sequence error: no resident witness: " + self._ctx()
        self._fresh("prove_dev(witness_buffer)", (), [ri])
        self._proof(self.resident, ri, self.pr.prove_dev(*self.cfg.rs_ints[ri], self.pr.witness_buffer()).raw)

    def prove_dev_own(self, wi, ri):
        """from the caller's own device buffer: a torch tensor on the GPU, host memory on the emulator"""
        self._fresh("prove_dev(own buffer)", [wi], [ri])
        wm = self.cfg.w_mont[wi]
        if self.cfg.emu:
            keep, ptr = wm, wm.ctypes.data
        else:
            import torch
            keep = torch.from_numpy(wm.view(np.int64)).cuda()
            torch.cuda.synchronize()
            ptr = keep.data_ptr()
        self.keep.append(keep)
        if self.multi:
            self.resident = None       # the peer broadcast lands in the staging buffers
        self._proof(wi, ri, self.pr.prove_dev(*self.cfg.rs_ints[ri], ptr).raw)

    # -- calls that take no witness
    def msm(self, q, si):
        self._fresh(f"msm_g2[{si}]" if q == QUERY_B2 else f"msm_g1({q})[{si}]", (), (), [(q, si)])
        sc = H.fr_mont_arr(self.cfg.scalars[q][si])
        got = self.pr.msm_g2(sc) if q == QUERY_B2 else self.pr.msm_g1(q, sc)
        assert got == self.cfg.want_msm(q, si), f"MSM over query {q}, scalar vector {si}: " + self._ctx()

    def msm_refused_too_long(self):
        self.ops.append("msm_g1(too many scalars)")
        self._refused(self.pr.msm_g1, QUERY_A, np.zeros((self.cfg.n_vars, 4), dtype=np.uint64))

    def prove_refused_short(self):
        self.ops.append("prove(short witness)")
        self._refused(self.pr.prove, 1, 2, self.cfg.w_mont[0][:-1])

    def info(self):
        self.ops.append("info")
        assert self.pr.info()["domain_size"] == self.cfg.domain, self._ctx()

    def profiling(self, on):
        self.ops.append(f"set_profiling({on})")
        self.pr.set_profiling(on)

    def stage_times(self):
        self.ops.append("stage_times")
        t = self.pr.stage_times()
        assert t and all(ms >= 0 and cnt >= 0 for ms, cnt in t.values()), self._ctx()

    # -- the witness map and the batch calls
    def witness_map(self, wi):
        self._fresh("witness_map", [wi])
        self.resident = None
        assert np.array_equal(self.pr.witness_map(self.cfg.w_mont[wi]), self.cfg.want_h(wi)), \
            f"h of witness {self.cfg.w_names[wi]}: " + self._ctx()

    def witness_map_batch(self, wis):
        self._fresh(f"witness_map_batch({len(wis)})", wis)
        self.resident = None
        h = self.pr.witness_map_batch(np.stack([self.cfg.w_mont[wi] for wi in wis]))
        for i, wi in enumerate(wis):
            assert np.array_equal(h[i], self.cfg.want_h(wi)), f"h {i} of the batch ({self.cfg.w_names[wi]}): " + self._ctx()

    def prove_batch(self, combos, canonical=False):
        self._fresh(f"prove_wtns_batch({len(combos)})" if canonical else f"prove_batch({len(combos)})",
                    [wi for wi, _ in combos], [ri for _, ri in combos])
        self.resident = None
        rs = [self.cfg.rs_ints[ri] for _, ri in combos]
        if canonical:
            got = self.pr.prove_wtns_batch([self.cfg.w_le[wi] for wi, _ in combos], rs)
        else:
            got = self.pr.prove_batch(rs, np.stack([self.cfg.w_mont[wi] for wi, _ in combos]))
        assert len(got) == len(combos), self._ctx()
        for (wi, ri), p in zip(combos, got):
            self._proof(wi, ri, p.raw)

    def verify_one(self):
        """one proof of a satisfying witness of this sequence: pairing-verified, rejected for a wrong input"""
        sat = [(wi, raw) for wi, raw in self.proofs if wi in SAT]
        assert sat, "sequence error: no proof of a satisfying witness: " + self._ctx()
        assert self.cfg.verify(*sat[-1]), "a proof equal to the CPU restatement's does not verify: " + self._ctx()


def _on(*names):
    """the cases of a scripted sequence: each configuration on the emulator and on the GPU, as the `lib` fixture
    parametrises them.  The emulator builds the fixed-base tables of even a 16-wire key in most of a minute: the
    T cases there carry the slow mark (and share one donor's tables, see Session)."""
    out = []
    for name in names:
        if CONFIGS[name][0] is not None:
            out.append(pytest.param("emu", name, marks=[pytest.mark.slow] if name == "T" else [], id=f"emu-{name}"))
        out.append(pytest.param("gpu", name, marks=pytest.mark.gpu, id=f"gpu-{name}"))
    return pytest.mark.parametrize("where,name", out, indirect=["where"])


@pytest.fixture
def where(request):
    return request.getfixturevalue("emu" if request.param == "emu" else "gpulib")


@pytest.fixture
def session(where):
    lib, made = where, []

    def make(name, label="", **kw):
        s = Session(config(name, lib), label, **kw)
        made.append(s)
        return s
    yield make
    for s in made:
        s.close()


# ---- scripted sequences: one per named hazard ---------------------------------------------------------------------
@_on("T", "B")
def test_resident_witness_survives_calls_that_take_no_witness(session, name):
    """1. upload_witness(w1), then the calls that take no witness -- msm_g1 over A (full length), over H, msm_g2
    (full length, other scalars), info, set_profiling -- then prove_dev from witness_buffer(): the proof of w1.
    Again after two refused calls (a short witness, too many scalars), and again after another upload."""
    s = session(name)
    deal = Deal(s.cfg, 1)
    w1, r1 = deal()
    s.upload(w1)
    s.msm(QUERY_A, 0)
    s.msm(QUERY_H, 0)
    s.msm(QUERY_B2, 0)
    s.info()
    s.profiling(True)
    s.prove_resident(r1)
    s.prove_refused_short()
    s.msm_refused_too_long()
    s.prove_resident(deal()[1])
    s.upload(deal()[0], canonical=True)
    s.msm(QUERY_B1, 1)
    s.msm(QUERY_L, 0)
    s.prove_resident(deal()[1])
    s.verify_one()


@_on("B", "R")
def test_sort_shrinks_and_grows_between_calls(session, name):
    """2. the entry count of the witness sort from call to call: dense (every entry), one scalar, zeros (w[0] = 1
    alone: no entry at all), the whole L query, a skewed vector (hot buckets), two scalars on G2, dense again"""
    s = session(name)
    s.prove(3, 3)            # dense0
    s.msm(QUERY_A, 1)        # one scalar
    s.prove(5, 5)            # zeros
    s.msm(QUERY_L, 0)        # full length
    s.prove(4, 4)            # skewed0
    s.msm(QUERY_B2, 2)       # length 2
    s.prove(6, 6)            # dense1
    s.prove(7, 0)            # all r - 1: one bucket per window; (r, s) = (0, 0)
    s.prove(1, 1)            # a satisfying witness
    s.verify_one()


@_on("T", "B")
def test_every_way_a_witness_arrives_alternating(session, name):
    """3. host, the caller's device buffer, upload + prove_dev twice, canonical, canonical refused, host, canonical
    upload + prove_dev: each with another witness and another (r, s)"""
    s = session(name)
    deal = Deal(s.cfg, 2)
    s.prove(*deal())
    s.prove_dev_own(*deal())
    wi, ri = deal()
    s.upload(wi)
    s.prove_resident(ri)
    s.prove_resident(deal()[1])
    s.prove_wtns(*deal())
    s.prove_wtns_refused(*deal())
    s.prove(*deal())
    wi, ri = deal()
    s.upload(wi, canonical=True)
    s.prove_resident(ri)
    s.prove(*deal())
    s.verify_one()


@_on("T", "B")
def test_batch_workspace_grows_between_single_proofs(session, name):
    """4. the batch workspace is allocated by a batch of 2, regrown by a batch of 5, used by the witness-map batch,
    by a batch of 1 and by a canonical batch of 4, with single proofs before, between and behind"""
    s = session(name)
    assert s.pr.info()["batched"] == 1
    deal = Deal(s.cfg, 0)
    s.prove_batch(deal(2))
    s.prove(*deal())
    s.prove_batch(deal(5))
    s.witness_map_batch([w for w, _ in deal(3)])
    s.prove_batch(deal(1))
    s.prove_batch(deal(4), canonical=True)
    s.prove(*deal())
    s.verify_one()


@_on("T", "B", "WM")
def test_witness_map_and_h_staging_between_proofs(session, name):
    """5. g16_witness_map and the H-query MSM stage in h_dev, which a proof's witness map writes too.  On the
    witness-map-only ctx the proving calls are refused and the maps around them still give the oracle's h."""
    s = session(name)
    wm_only = name == "WM"
    if wm_only:
        s.prove_refused = lambda wi, ri: (s.ops.append("prove(no key)"), s._refused(
            s.pr.prove, *s.cfg.rs_ints[ri], s.cfg.w_mont[wi]))
        s.prove_refused(0, 3)
    else:
        s.prove(0, 3)
    s.witness_map(3)
    if wm_only:
        s.ops.append("msm_g1(no key)")
        s._refused(s.pr.msm_g1, QUERY_H, H.fr_mont_arr(s.cfg.scalars[QUERY_H][0]))
    else:
        s.msm(QUERY_H, 1)
    s.witness_map(5)          # zeros: h = 0 after an h of full-width values
    if wm_only:
        s.prove_refused(4, 7)
    else:
        s.prove(4, 7)
        s.msm(QUERY_H, 2)     # three scalars after a whole h
    s.witness_map_batch([7, 1])
    s.witness_map(8)
    if not wm_only:
        s.prove(2, 5)
        s.verify_one()


@pytest.mark.parametrize("shard", ["points", "buckets"])
@_on("W2")
def test_sharded_finish_rs_cache_miss_recompute_and_hit(session, name, shard):
    """6. rank_partial_enqueue leaves the (r, s)-only sums of ITS (r, s) on the side stream (fixed_ready, fixed_rs).
    Two rounds of partials, then finish for the FIRST round's pair: the cached pair is the second round's (the miss
    path); finish for the second pair after the flag was cleared (recomputed); then a round with the same pair
    and a new witness, finished at once: the hit path."""
    ranks = [session(name, f"rank {g} {shard}", rank=g, world=2, shard=shard) for g in range(2)]
    cfg = ranks[0].cfg
    assert all(s.pr.info()["shard_mode"] == shard for s in ranks)

    def partials(wi, ri):
        out = b""
        for s in ranks:
            s.ops.append(f"prove_partial(w{wi}, rs{ri})")
            out += s.pr.prove_partial(*cfg.rs_ints[ri], cfg.w_mont[wi])
        return out

    def finish(wi, ri, parts):
        s = ranks[0]
        s.ops.append(f"prove_finish(rs{ri})")
        s._proof(wi, ri, s.pr.prove_finish(*cfg.rs_ints[ri], parts).raw)
    p1 = partials(3, 3)
    p2 = partials(4, 4)
    finish(3, 3, p1)
    finish(4, 4, p2)
    p3 = partials(1, 4)       # the same (r, s), another witness
    finish(1, 4, p3)
    p4 = partials(5, 0)       # zeros with (0, 0): the finish of an all-infinity record behind a full one
    finish(5, 0, p4)
    ranks[0].verify_one()


@_on("M")
def test_multi_device_ctx_changing_witnesses(session, name):
    """7. devices = [0, 0]: host, resident, the caller's buffer (peer broadcast), host, canonical resident -- the
    moves of test_in_library_multi_device_prover with another witness and (r, s) each time"""
    s = session(name)
    deal = Deal(s.cfg, 1)
    s.prove(*deal())
    wi, ri = deal()
    s.upload(wi)
    s.prove_resident(ri)
    s.prove_dev_own(*deal())
    s.prove(*deal())
    wi, ri = deal()
    s.upload(wi, canonical=True)
    s.prove_resident(ri)
    s.prove_resident(deal()[1])
    s.prove_wtns(*deal())
    s.verify_one()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["B", "R"])
def test_profiling_toggled_between_proofs(gpulib, name):
    """8. the profiling switch puts timer events into every stream: on, proof, read, off, proof, on, a batch"""
    s = Session(config(name, gpulib))
    try:
        deal = Deal(s.cfg, 3)
        s.profiling(True)
        s.prove(*deal())
        s.stage_times()
        s.profiling(False)
        s.prove(*deal())
        s.profiling(True)
        s.prove_batch(deal(3))
        s.stage_times()
        s.profiling(False)
        s.prove(1, 1)
        s.verify_one()
    finally:
        s.close()


@_on("S")
def test_sparse_b_view_across_zero_patterns(session, name):
    """9. the filtered B view (MsmSort::run_view) is rebuilt from each witness sort: four witnesses whose zero
    patterns differ, a G2 MSM over the whole query and one of a single scalar between them"""
    s = session(name)
    s.prove(0, 3)
    s.prove(5, 5)            # zeros
    s.msm(QUERY_B2, 0)       # the whole query: the same entry count as a proof's sort
    s.prove(4, 4)            # skewed
    s.msm(QUERY_B2, 1)       # one scalar
    s.prove(3, 6)            # dense
    s.msm(QUERY_A, 0)
    s.prove(1, 1)
    s.verify_one()


@_on("F")
def test_fix_list_does_not_carry_over_between_launches(session, name):
    """10. the list of set-aside additions is filled by one launch and must be empty for the next: witnesses and
    scalars with many equal entries over a key of equal points (every launch defers, the list does not overflow)
    alternate with dense ones (no launch defers).  test_optimistic_accumulation_overflow_... covers the overflowed
    list, after which every launch takes the exact kernel."""
    s = session(name)
    assert s.pr.info()["c_w"] == 16
    s.prove(0, 0)            # ones
    s.prove(3, 3)            # dense
    s.msm(QUERY_A, 2)        # skewed
    s.msm(QUERY_A, 0)        # dense
    s.msm(QUERY_L, 1)        # skewed
    s.msm(QUERY_H, 2)        # three scalars
    s.prove(1, 1)            # twos
    s.prove(5, 5)            # zeros
    s.prove(2, 2)            # ones with a few full-width entries
    s.prove(6, 6)            # dense


# ---- seeded walks (GPU) -------------------------------------------------------------------------------------------
def _walk(s, seed, steps=40):
    """40 operations drawn by random.Random(seed) from every single-ctx call of the sequences above, refused calls
    included; a pure function of (config, seed)"""
    cfg = s.cfg
    rng = random.Random(f"{cfg.name} walk {seed}")
    s.label = f"seed {seed}"

    def combos(k):
        """k combinations that differ from each other and from the previous step in witness and (r, s)"""
        pool = list(cfg.combos)
        rng.shuffle(pool)
        out, ws, rs = [], set(s.last["w"]), set(s.last["rs"])
        for wi, ri in pool:
            if wi not in ws and ri not in rs:
                out.append((wi, ri))
                ws.add(wi)
                rs.add(ri)
                if len(out) == k:
                    return out
        if not out:           # (none of the listed combinations is free: any free pair)
            out = [(rng.choice([w for w in range(NW) if w not in ws]), rng.choice([r for r in range(NRS) if r not in rs]))]
        return out            # fewer than asked for: the batch is that much smaller

    def an_rs():
        return rng.choice([ri for ri in sorted({r for w, r in cfg.combos if w == s.resident}) if ri not in s.last["rs"]]
                          or [None])

    def a_scalar(q):
        return rng.choice([si for si in range(len(cfg.scalars[q])) if (q, si) not in s.last["sc"]])

    ops = ["prove", "prove", "prove_dev_own", "upload", "upload_canonical", "prove_resident", "prove_resident",
           "prove_wtns", "prove_wtns_refused", "msm_a", "msm_b1", "msm_l", "msm_h", "msm_g2", "info", "profiling",
           "stage_times", "prove_refused_short", "msm_refused_too_long", "prove_batch", "prove_wtns_batch",
           "witness_map", "witness_map_batch"]
    on = False
    for _ in range(steps):
        op = rng.choice(ops)
        if op == "prove_resident":
            ri = an_rs() if s.resident is not None else None
            if ri is None:
                op = "upload"
            else:
                s.prove_resident(ri)
                continue
        if op in ("prove", "prove_dev_own", "prove_wtns", "prove_wtns_refused"):
            getattr(s, op)(*combos(1)[0])
        elif op in ("upload", "upload_canonical"):
            s.upload(combos(1)[0][0], canonical=op == "upload_canonical")
        elif op.startswith("msm_") and op != "msm_refused_too_long":
            q = dict(msm_a=QUERY_A, msm_b1=QUERY_B1, msm_l=QUERY_L, msm_h=QUERY_H, msm_g2=QUERY_B2)[op]
            s.msm(q, a_scalar(q))
        elif op == "profiling":
            on = not on
            s.profiling(on)
        elif op in ("prove_batch", "prove_wtns_batch"):
            s.prove_batch(combos(rng.randrange(1, 6)), canonical=op == "prove_wtns_batch")
        elif op == "witness_map":
            s.witness_map(combos(1)[0][0])
        elif op == "witness_map_batch":
            s.witness_map_batch([w for w, _ in combos(rng.randrange(1, 4))])
        else:
            getattr(s, op)()
    # the walk ends on a satisfying witness, which is pairing-verified
    wi, ri = next(c for c in cfg.combos if c[0] in SAT and c[0] not in s.last["w"] and c[1] not in s.last["rs"])
    s.prove(wi, ri)
    s.verify_one()


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("name", ["T", "B", "R", "S"])
def test_seeded_walk(gpulib, name, seed):
    s = Session(config(name, gpulib))
    try:
        _walk(s, seed)
    finally:
        s.close()


@pytest.mark.gpu
def test_sibling_ctxs_prove_different_witnesses_in_flight(gpulib):
    """test_sibling_ctx_two_proofs_in_flight with witnesses that differ between the two ctxs and from iteration to
    iteration: a donor and its sibling (config R) on one host thread each, six proofs each"""
    cfg = config("R", gpulib)
    donor = Session(cfg, "donor")
    sib = Session(cfg, "sibling", sibling_of=donor.pr)
    for wi, ri in cfg.combos[:12]:       # the expected values, before the threads start
        cfg.want_proof(wi, ri)
    errors = []

    def run(s, mine):
        try:
            for wi, ri in mine:
                s.prove(wi, ri)
        except BaseException as e:     # noqa: B036 -- handed to the main thread
            errors.append(e)
    # iteration i: the donor proves combination i, the sibling combination i + 6 (another witness, another (r, s))
    ths = [threading.Thread(target=run, args=(donor, cfg.combos[0:6])),
           threading.Thread(target=run, args=(sib, cfg.combos[6:12]))]
    try:
        for t in ths:
            t.start()
        for t in ths:
            t.join()
        if errors:
            raise errors[0]
        assert len(donor.proofs) == 6 and len(sib.proofs) == 6
        donor.verify_one()
    finally:
        sib.close()
        donor.close()
