"""The host code that reads untrusted bytes — zkir_amd/csrc/verify.cpp, interp.cpp, hashes.cpp and the host parts of hashcall.h, verify_stages.h, host.h — run under
AddressSanitizer and UndefinedBehaviorSanitizer on honest and malformed input.  CPU only.

A read a few words past a numpy buffer does not crash and undefined behaviour does not show through ctypes, so the fuzz tests that call the library from Python
(tests/test_verifier.py, tests/test_stark_mode4.py) can compare verdicts but cannot see memory errors.  Code loaded into Python cannot be run under a sanitizer either.  So
the three host sources are compiled a second time, with -fsanitize=address,undefined, and linked with a stand-alone program (tests/cpp/host_san_driver.cpp) that reads a
corpus file, copies every input buffer into a heap block of exactly its length (the word behind it is a redzone) and prints one verdict line per case.  LeakSanitizer stays
on: a leak on an error path is a finding.

The corpus is made here, with a fixed seed, from the CPU oracle's proofs and the Python references: honest proofs of modes 0 .. 4, chains of segments, low-degree proofs,
opening records, hash and wide tapes, program blobs — and mutants of each: header and count words at edge values, counts that make a section end at / before / past the
proof's end, truncations at every section boundary, extensions, swaps, zeroed runs.  Asserted per family: the driver exits 0 with no sanitizer report; every honest original
is accepted; every mutant that differs from its original is rejected; every verdict is the oracle's for the same bytes (so.verify / verify_chain / verify_io,
lowdeg_ref.verify_ref, merkle_open_ref.verify_all_ref, tape_side_ref.expected_check_code / reference, tape_digest_ref.expected_new_bytes, oracle.run); the rejection codes
of a family span at least four values (opening records and blobs have no such codes: their tests say what stands in).

The driver links no HIP object, so the bodies of the entry points that the library defines in its HIP translation units are not run.  zkir_interpret and
zkir_hash_tape_check_host are covered through the host functions they forward to.  Of zkir_hash_tape_new_bytes_host the parser and the per-call function run, in a serial
loop: not its threaded copy into the caller's array.  zkir_tape_table_side_host's body (tape_table.inl's host sums over the caller's new_bytes) is not sanitized at all: in
its place run the verifier's host tape stages of verify.cpp / verify_stages.h, which read the same sections in zkir_verify and form the same sum by other code (see the
driver's head comment).  The driver's restatement of zkir_padded_log_n is held against the library's below."""
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import lowdeg_ref as LD
import merkle_open_ref as MO
import programs as pg
import tape_digest_ref as TD
import tape_side_ref as TS
from oracle import api as oracle, stark_api as so
from zkir_amd import build as zbuild, spec, stark

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = os.path.join(ROOT, "tests", "cpp", "_san")
DRIVER_SRC = os.path.join(ROOT, "tests", "cpp", "host_san_driver.cpp")
BIN = os.path.join(SAN, "host_san_driver")
SAN_FLAGS = ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
P = so.P
U64_MAX = (1 << 64) - 1
EDGES = [0, 1, 1 << 16, (1 << 20) - 1, (1 << 20) + 1, 1 << 24, 1 << 28, (1 << 30) - 1, (1 << 30) + 1, P - 1, P, 1 << 31, 0xFFFFFFFF]
(VERIFY, VERIFY_SEGMENT, VERIFY_CHAIN, VERIFY_IO, VERIFY_CHAIN_IO, LOWDEG, MERKLE, HASH_CHECK, TAPE_SIDE, NEW_BYTES, CALL_CELLS, DIGEST_BYTES, INTERPRET,
 PADDED_LOG_N) = range(14)


# ---- the build -------------------------------------------------------------------------------------------------------------------------------------------------------------
def _linker():
    """the clang++ beside hipcc's compiler: the link line takes objects only, and the driver is to link no HIP runtime"""
    for cand in (os.path.join(os.path.dirname(os.path.realpath(zbuild.HIPCC)), "..", "llvm", "bin", "clang++"), "/opt/rocm/llvm/bin/clang++"):
        if os.path.exists(cand):
            return os.path.normpath(cand)
    return zbuild.HIPCC


@pytest.fixture(scope="module")
def driver():
    os.makedirs(SAN, exist_ok=True)
    probe = os.path.join(SAN, "probe.cpp")
    with open(probe, "w") as f:
        f.write("#include <vector>\nint main() { std::vector<int> v(3, 1); return v[0] + v[2] - 2; }\n")
    p = subprocess.run([zbuild.HIPCC, "-x", "c++", *SAN_FLAGS, probe, "-o", os.path.join(SAN, "probe")], capture_output=True, text=True)
    if p.returncode != 0 or subprocess.run([os.path.join(SAN, "probe")], capture_output=True).returncode != 0:
        pytest.skip("the compiler cannot link or run a program with the AddressSanitizer / UndefinedBehaviorSanitizer runtime: " + p.stderr[-300:])
    deps = [os.path.normpath(os.path.join(zbuild.CSRC, h)) for h in zbuild.HEADERS]
    objs, jobs = [], []
    for src in [os.path.join(zbuild.CSRC, name) for name in zbuild.HOST_SOURCES] + [DRIVER_SRC]:
        obj = os.path.join(SAN, os.path.basename(src) + ".o")
        objs.append(obj)
        if zbuild._newer(src, obj, deps):
            jobs.append(subprocess.Popen([zbuild.HIPCC, "-x", "c++", "-std=c++17", *SAN_FLAGS, "-Wall", "-Wno-unused-function", "-c", src, "-o", obj]))
    for j in jobs:                                                   # (the translation units are independent: side by side)
        assert j.wait() == 0, "a sanitizer build of a host source failed"
    if zbuild._newer(objs[0], BIN, objs[1:]):
        subprocess.check_call([_linker(), "-fsanitize=address,undefined", *objs, "-o", BIN])
    return BIN


# ---- the corpus ------------------------------------------------------------------------------------------------------------------------------------------------------------
class Corpus:
    """Cases for the driver and the verdict the oracle expects of each.  A buffer is a numpy array, or (base id, array): written as the base's prefix + patches + a tail."""

    def __init__(self, name):
        self.name, self.bases, self.cases = name, [], []

    def base(self, arr):
        self.bases.append(np.ascontiguousarray(arr))
        return len(self.bases) - 1

    def add(self, label, kind, args, bufs, want, mutant=False, accepted=None):
        """want: the verdict line, or its leading words; accepted: whether `want` is an acceptance (mutants must not be)"""
        self.cases.append(dict(label=label, kind=kind, args=[int(a) for a in args], bufs=bufs, want=want, mutant=mutant, accepted=accepted))

    def _buf(self, b):
        base, arr = b if isinstance(b, tuple) else (None, b)
        arr = np.ascontiguousarray(arr)
        elem = arr.dtype.itemsize
        take, patches, tail = 0, np.zeros((0, 2), "<u8"), arr
        if base is not None:
            ref = self.bases[base]
            assert ref.dtype == arr.dtype
            n = min(len(ref), len(arr))
            diff = np.nonzero(ref[:n] != arr[:n])[0]
            if 4 * len(diff) <= n:
                take, tail = n, arr[n:]
                patches = np.stack([diff.astype("<u8"), arr[diff].astype("<u8")], axis=1)
        return (struct.pack("<IIQQ", elem, 0xFFFFFFFF if not take else base, take, len(patches)) + patches.astype("<u8").tobytes() + struct.pack("<Q", len(tail))
                + tail.astype(arr.dtype.newbyteorder("<")).tobytes())

    def write(self, path):
        with open(path, "wb") as f:
            f.write(struct.pack("<II", 0x43534B5A, len(self.bases)))
            for b in self.bases:
                f.write(struct.pack("<IQ", b.dtype.itemsize, len(b)) + b.astype(b.dtype.newbyteorder("<")).tobytes())
            f.write(struct.pack("<I", len(self.cases)))
            for c in self.cases:
                f.write(struct.pack("<II", c["kind"], len(c["args"])) + b"".join(struct.pack("<Q", a & U64_MAX) for a in c["args"]) + struct.pack("<I", len(c["bufs"])))
                for b in c["bufs"]:
                    f.write(self._buf(b))


def _check(binary, corpus, min_codes=0):
    """Runs the driver on the corpus: no sanitizer report, exit 0, every verdict the expected one, every mutant rejected, the rejection codes spread."""
    path = os.path.join(SAN, f"corpus_{corpus.name}.bin")
    corpus.write(path)
    env = {k: v for k, v in os.environ.items() if k not in ("ASAN_OPTIONS", "UBSAN_OPTIONS", "LSAN_OPTIONS")}      # the sanitizers' defaults: every check on
    p = subprocess.run([binary, path], capture_output=True, text=True, env=env, timeout=1500)
    for marker in ("AddressSanitizer", "LeakSanitizer", "runtime error:", "UndefinedBehaviorSanitizer"):
        assert marker not in p.stderr, f"{corpus.name}: sanitizer report\n" + p.stdout[-400:] + "\n" + p.stderr[:6000]
    assert p.returncode == 0, (corpus.name, p.returncode, p.stderr[-2000:])
    lines = p.stdout.splitlines()
    assert len(lines) == len(corpus.cases), (corpus.name, len(lines), len(corpus.cases))
    wrong, codes = [], {}
    for i, (line, c) in enumerate(zip(lines, corpus.cases)):
        got, want = line.split(" | ")[0], f"{i} {c['want']}"
        if not (got == want or got.startswith(want + " ")):
            wrong.append((c["label"], got, want))
        if c["mutant"]:
            assert c["accepted"] is False, ("a mutant that differs from its original is accepted", corpus.name, c["label"], c["want"])
            codes[c["want"]] = codes.get(c["want"], 0) + 1
    assert not wrong, (corpus.name, len(wrong), wrong[:8])
    assert len(codes) >= min_codes, (corpus.name, "the rejections collapse into few codes", codes)
    os.remove(path)
    return codes


def _expect_words(pub):
    return np.array([pub.n_real, pub.entry, pub.deferred, pub.fri, *pub.prog, *pub.io], np.uint64)


def _same(a, b):
    return len(a) == len(b) and np.array_equal(a, b)


# ---- mutants of a proof ----------------------------------------------------------------------------------------------------------------------------------------------------
def _proof_sections(proof):
    """(the count and length words of a proof of any mode: [(name, position, proof words per unit counted)], its section boundaries), from stark.proof_layout"""
    lay = stark.proof_layout(proof)
    mode, n = lay["mode"], len(proof)
    hw = stark.HEADER_WORDS + (4 if mode >= 2 else 0)
    counts = [("blob_len", hw, 0.5)]
    bounds = [stark.HEADER_WORDS, hw, hw + 1, lay["rom_mult"], lay["rc_mult"], lay["trace_root"], lay["aux_root"], lay["quotient_root"], lay["openings"]]
    if mode >= 2:
        io = lay["io_section"]
        n_in = int(proof[io])
        out_at = io + 1 + 4 * n_in
        counts += [("n_in", io, 4), ("n_out", out_at, 4), ("halt_kind", out_at + 1 + 4 * int(proof[out_at]), 1)]
        bounds += [io, out_at, out_at + 1 + 4 * int(proof[out_at])]
    if mode >= 3:
        counts.append(("n_cells", lay["mem_section"], 7)); bounds.append(lay["mem_section"])
    if mode == 4:
        at = lay["hash_section"]
        counts.append(("n_calls", at, 28)); bounds += [at, lay["wide_section"]]
        q = at + 1
        for k in range(int(proof[at])):
            if k < 3:
                counts += [(f"call{k}_len", q + 3, 1), (f"call{k}_cells", q + 7, 5)]
            bounds.append(q)
            q += 8 + 5 * int(proof[q + 7])
        counts.append(("n_wide", lay["wide_section"], 8))
    wt = int(proof[3]) + so.aux_width(mode)
    layers_at = lay["openings"] + 4 * (2 * wt + 4)
    n_layers = int(proof[layers_at])
    queries = layers_at + 1 + 4 * n_layers + 4 * 8 + 1
    nq = int(proof[4])
    qsize = (n - queries) // nq
    assert queries + nq * qsize == n
    counts.append(("n_layers", layers_at, 4))
    counts += [(f"query{t}", queries + t * qsize, 1) for t in (0, 1, nq - 1)]
    bounds += [layers_at, layers_at + 1, queries - 1, queries, queries + 1, queries + qsize, queries + (nq - 1) * qsize]
    return counts, sorted(set(bounds))


def _proof_mutants(proof, rng, n_random=60):
    """[(label, words)]: the mutant classes of the module's docstring on one proof"""
    n = len(proof)
    counts, bounds = _proof_sections(proof)
    out = []

    def put(label, pos, val):
        t = proof.copy(); t[pos] = val & 0xFFFFFFFF
        out.append((label, t))
    header = list(range(0, 21)) + [int(x) for x in rng.integers(21, stark.HEADER_WORDS, 6)] + list(range(stark.HEADER_WORDS, stark.HEADER_WORDS + (4 if proof[9] >= 2 else 0)))
    for pos in header:                                              # header and parameter words at the edges
        for v in EDGES:
            put(f"header{pos}={v}", pos, v)
    for name, pos, unit in counts:                                  # every count / length word: the edges, and the values that end its section at / before / past the proof's end
        k = int((n - pos - 1) / unit)
        for v in EDGES + [k - 2, k - 1, k, k + 1, k + 2, int(proof[pos]) + 1, max(int(proof[pos]) - 1, 0)]:
            put(f"{name}={v}", pos, max(v, 0))
    for b in bounds + [n]:                                          # truncation at every section boundary - 1, + 0, + 1
        for cut in (b - 1, b, b + 1):
            if 0 <= cut <= n:
                out.append((f"cut{cut}", proof[:cut].copy()))
    for cut in rng.integers(0, n, n_random // 2):
        out.append((f"cut{cut}", proof[:int(cut)].copy()))
    for extra in (1, 2, 7, 40):                                     # extension
        out.append((f"extend{extra}", np.concatenate([proof, rng.integers(0, P, extra).astype(np.uint32)])))
    out.append(("extend_zero", np.concatenate([proof, np.zeros(1, np.uint32)])))
    for _ in range(n_random):                                       # any word, any value; swaps; zeroed runs
        put("word", int(rng.integers(0, n)), int(rng.integers(0, 1 << 32)))
        a, b = (int(x) for x in rng.integers(0, n, 2))
        t = proof.copy(); t[a], t[b] = t[b], t[a]
        out.append((f"swap{a},{b}", t))
        a = int(rng.integers(0, n))
        t = proof.copy(); t[a:a + int(rng.integers(1, 64))] = 0
        out.append((f"zero{a}", t))
    return [(label, t) for label, t in out if not _same(t, proof)]


def _run_of(blob, ins=(), **cfg):
    return oracle.run(blob, list(ins), enable_execution_trace=True, **cfg)


def _honest_proof(mode):
    """an oracle proof of the mode at a small row count, its public inputs"""
    kw = {}
    if mode == 0:
        blob, ins = spec.fib_endless_program().to_bytes(), []
        res = _run_of(blob, max_cycles=40)
    elif mode == 1:
        blob, ins = spec.fib_endless_program().to_bytes(), []
        res = _run_of(blob, max_cycles=37, enable_deferred_model=True); kw = dict(deferred=True)
    elif mode == 2:
        blob, ins, _ = pg.echo5()
        res = _run_of(blob, ins); kw = dict(io_mode=True)
    elif mode == 3:
        blob, ins, _ = pg.off_code("timestamps")
        res = _run_of(blob, ins); kw = dict(mem_mode=True)
    else:
        blob, ins, _ = TS.wide_and_hash_program()
        res = _run_of(blob, ins); kw = dict(wide_mode=True)
    pub = so.public_inputs(len(res.rows), blob, list(ins), list(res.outputs), (res.halt_kind, res.halt_code), **kw)
    return so.prove(res.rows, pub), pub


@pytest.mark.parametrize("mode", [0, 1, 2, 3, 4])
def test_zkir_verify_on_mutated_proofs(driver, mode):
    """zkir_verify, with and without `expect`, on about 1000 mutants of an honest proof of the mode (mode 4: a run with touched cells, a hash tape and a wide tape)."""
    proof, pub = _honest_proof(mode)
    lay = stark.proof_layout(proof)
    assert lay["mode"] == mode and proof[9] == mode
    if mode == 4:
        assert proof[lay["mem_section"]] >= 1 and proof[lay["hash_section"]] >= 1 and proof[lay["wide_section"]] >= 1
    c = Corpus(f"mode{mode}")
    b, e = c.base(proof), _expect_words(pub)
    assert so.verify(proof, pub) == 0 and so.verify(proof) == 0
    c.add("honest", VERIFY, [0], [(b, proof)], "rc 0")
    c.add("honest, expected", VERIFY, [1], [(b, proof), e], "rc 0")
    other = so.public_inputs(pub.n_real + 1, pub._blob_ref)
    assert so.verify(proof, other) != 0
    c.add("honest, another run expected", VERIFY, [1], [(b, proof), _expect_words(other)], f"rc {so.verify(proof, other)}")
    rng = np.random.default_rng(4100 + mode)
    for i, (label, t) in enumerate(_proof_mutants(proof, rng, n_random=130)):
        with_expect = i % 3 == 2
        want = so.verify(t, pub if with_expect else None)
        c.add(label, VERIFY, [int(with_expect)], [(b, t), e] if with_expect else [(b, t)], f"rc {want}", mutant=True, accepted=want == 0)
    assert len(c.cases) >= 900
    _check(driver, c, min_codes=4)
    print(f"mode {mode}: {len(c.cases)} cases, proof of {len(proof)} words")


def _chain(n_total, seg_rows):
    from test_stark_oracle import _segments
    return _segments(n_total, seg_rows)


def _mode2_chain():
    """echo5 proven in two mode-2 segments (the second one starts with WRITE / READ ecalls behind it)"""
    blob, ins, _ = pg.echo5()
    res = _run_of(blob, ins)
    n, cut = len(res.rows), len(res.rows) // 2
    ecalls = lambda num: sum(1 for r in res.rows[:cut] if (int(r["instruction"]) & 0x7F) == 0x50 and int(r["registers"][10]) == num)   # noqa: E731
    args = (blob, list(ins), list(res.outputs), (res.halt_kind, res.halt_code))
    run_pub = so.public_inputs(n, *args, io_mode=True)
    pubs = [so.public_inputs(cut + 1, *args, io_mode=True), so.public_inputs(n - cut, *args, io_mode=True, writes_before=ecalls(2), reads_before=ecalls(1))]
    for p in pubs:
        p.io[:] = list(run_pub.io)
    return [so.prove(res.rows[:cut + 1], pubs[0]), so.prove(res.rows[cut:], pubs[1])], run_pub, list(ins), list(res.outputs), (res.halt_kind, res.halt_code)


def _chain_mutants(proofs, rng, n):
    """[(label, segments)]: a damaged word, a header or count word at an edge, a truncated segment, segments dropped, repeated, reordered"""
    out = []
    for it in range(n):
        chain = [p.copy() for p in proofs]
        kind = it % 6
        k = int(rng.integers(0, len(chain)))
        if kind == 0:
            chain[k][int(rng.integers(0, len(chain[k])))] = int(rng.integers(0, 1 << 32))
        elif kind == 1:
            chain[k][int(rng.integers(0, 21))] = EDGES[int(rng.integers(0, len(EDGES)))]
        elif kind == 2:
            counts, bounds = _proof_sections(proofs[k])
            if rng.integers(0, 2):
                _, pos, unit = counts[int(rng.integers(0, len(counts)))]
                chain[k][pos] = max(int((len(chain[k]) - pos - 1) / unit) + int(rng.integers(-1, 2)), 0)
            else:
                chain[k] = chain[k][:max(bounds[int(rng.integers(0, len(bounds)))] + int(rng.integers(-1, 2)), 0)]
        elif kind == 3:
            chain[k] = chain[k][:int(rng.integers(0, len(chain[k])))]
        elif kind == 4:
            chain = chain[:k] + chain[k + 1:] if rng.integers(0, 2) else chain[:k] + [chain[k]] + chain[k:]
        else:
            chain = [chain[i] for i in rng.permutation(len(chain))]
        if chain and not (len(chain) == len(proofs) and all(_same(a, b) for a, b in zip(chain, proofs))):
            out.append((f"chain{it}/{kind}", chain))
    return out


def _is_prefix(chain, proofs):
    """the first segments of a chain are a chain themselves — of a shorter run: only the expected public inputs tell them from the whole"""
    return len(chain) < len(proofs) and all(_same(a, b) for a, b in zip(chain, proofs))


def _chain_bufs(bases, proofs, chain):
    """every segment of a damaged chain against the honest segment it resembles most (same position, else the first)"""
    return [(bases[i] if i < len(proofs) and len(s) == len(proofs[i]) else bases[int(np.argmin([abs(len(s) - len(p)) for p in proofs]))], s) for i, s in enumerate(chain)]


def test_chains_and_segments(driver):
    """zkir_verify_chain and zkir_verify_segment on a four-segment chain and on a two-segment chain of mode 2 (the tapes linked across segments), about 500 damaged copies."""
    c = Corpus("chain")
    rng = np.random.default_rng(4200)
    _, full, _, proofs = _chain(61, 16)
    assert len(proofs) == 4 and so.verify_chain(proofs, full) == 0
    bases = [c.base(p) for p in proofs]
    e = _expect_words(full)
    honest = [(bases[i], p) for i, p in enumerate(proofs)]
    c.add("honest", VERIFY_CHAIN, [0, 4], honest, "rc 0")
    c.add("honest, expected", VERIFY_CHAIN, [1, 4], honest + [e], "rc 0")
    for i, p in enumerate(proofs):
        rc, first, last = so.verify_segment(p)
        assert rc == 0
        c.add(f"segment{i}", VERIFY_SEGMENT, [0], [(bases[i], p)], f"rc 0 states {zlib.crc32(first.tobytes()):08x} {zlib.crc32(last.tobytes()):08x}")
        c.add(f"segment{i} as a run", VERIFY, [0], [(bases[i], p)], f"rc {so.verify(p)}")
    for i, (label, chain) in enumerate(_chain_mutants(proofs, rng, 330)):
        with_expect = int(i % 2 or _is_prefix(chain, proofs))
        want = so.verify_chain(chain, full if with_expect else None)
        c.add(label, VERIFY_CHAIN, [with_expect, len(chain)], _chain_bufs(bases, proofs, chain) + ([e] if with_expect else []), f"rc {want}", mutant=True, accepted=want == 0)
    for label, t in _proof_mutants(proofs[1], rng, n_random=10)[::12]:
        want = so.verify_segment(t)[0]
        c.add("segment " + label, VERIFY_SEGMENT, [0], [(bases[1], t)], f"rc {want}", mutant=True, accepted=want == 0)
    segs2, run_pub, ins, outs, halt = _mode2_chain()
    assert so.verify_chain(segs2, run_pub) == 0
    bases2 = [c.base(p) for p in segs2]
    c.add("honest mode 2", VERIFY_CHAIN, [1, 2], [(bases2[0], segs2[0]), (bases2[1], segs2[1]), _expect_words(run_pub)], "rc 0")
    e2 = _expect_words(run_pub)
    for label, chain in _chain_mutants(segs2, rng, 110):
        with_expect = int(_is_prefix(chain, segs2))
        want = so.verify_chain(chain, run_pub if with_expect else None)
        c.add("mode 2 " + label, VERIFY_CHAIN, [with_expect, len(chain)], _chain_bufs(bases2, segs2, chain) + ([e2] if with_expect else []), f"rc {want}", mutant=True, accepted=want == 0)
    assert len(c.cases) >= 450
    _check(driver, c, min_codes=4)
    print(f"chain: {len(c.cases)} cases")


def test_verify_io_and_chain_io(driver):
    """zkir_verify_io and zkir_verify_chain_io: the honest claim, every other claim, and about 500 damaged proofs and tapes."""
    c = Corpus("io")
    rng = np.random.default_rng(4300)
    u64 = lambda xs: np.array([int(x) & U64_MAX for x in xs], np.uint64)   # noqa: E731
    blob = spec.fib_program(12).to_bytes()
    res = _run_of(blob)
    halt = (res.halt_kind, res.halt_code)
    pub = so.public_inputs(len(res.rows), blob, [], list(res.outputs), halt)
    proof = so.prove(res.rows, pub)
    b, e = c.base(proof), _expect_words(pub)

    def io_case(label, t, with_expect, ins, outs, hk, mutant):
        want = so.verify_io(t, pub if with_expect else None, ins, outs, hk)
        c.add(label, VERIFY_IO, [int(with_expect), hk[0], hk[1]], [(b, t)] + ([e] if with_expect else []) + [u64(ins), u64(outs)], f"rc {want}", mutant=mutant, accepted=want == 0)
        return want
    assert io_case("honest", proof, True, [], [144], halt, False) == 0 and io_case("honest, no expect", proof, False, [], [144], halt, False) == 0
    claims = [([], [145], halt), ([7], [144], halt), ([], [144], (1, 1)), ([], [144], (0, 0)), ([], [144], (2, 0)), ([], [], halt), ([], [144, 144], halt), ([], [144], (3, 0)),
              ([], [144], (-1, 0)), ([], [144], (1, U64_MAX)), ([U64_MAX] * 9, [144], halt), ([], [U64_MAX], halt)]
    for k, (ins, outs, hk) in enumerate(claims):
        assert io_case(f"claim{k}", proof, bool(k & 1), ins, outs, hk, True) != 0
    for i, (label, t) in enumerate(_proof_mutants(proof, rng, n_random=20)[::2]):
        io_case(label, t, i % 2 == 0, [], [144], halt, True)
    # a run cut short and called an exit (52), the exit code of another run (53): proofs that verify, claims that do not hold
    k = len(res.rows) - 10
    pub_cut = so.public_inputs(k, blob, [], [144], (1, 0))
    cut = so.prove(res.rows[:k], pub_cut)
    want = so.verify_io(cut, pub_cut, [], [144], (1, 0))
    assert want == 52
    c.add("cut short", VERIFY_IO, [1, 1, 0], [cut, _expect_words(pub_cut), u64([]), u64([144])], "rc 52", mutant=True, accepted=False)
    pub5 = so.public_inputs(len(res.rows), blob, [], [144], (1, 5))
    code5 = so.prove(res.rows, pub5)
    assert so.verify_io(code5, pub5, [], [144], (1, 5)) == 53
    c.add("another exit code", VERIFY_IO, [1, 1, 5], [code5, _expect_words(pub5), u64([]), u64([144])], "rc 53", mutant=True, accepted=False)
    # the chain form: fib(12) in two segments
    n, half = len(res.rows), len(res.rows) // 2
    segs = []
    for lo, hi in ((0, half + 1), (half, n)):
        p = so.public_inputs(hi - lo, blob, [], list(res.outputs), halt)
        p.io[:] = list(pub.io)
        segs.append(so.prove(res.rows[lo:hi], p))
    bases = [c.base(s) for s in segs]

    def chain_case(label, chain, with_expect, ins, outs, hk, mutant):
        want = so.verify_chain_io(chain, pub if with_expect else None, ins, outs, hk)
        c.add(label, VERIFY_CHAIN_IO, [int(with_expect), len(chain), hk[0], hk[1]], _chain_bufs(bases, segs, chain) + ([e] if with_expect else []) + [u64(ins), u64(outs)], f"rc {want}",
              mutant=mutant, accepted=want == 0)
        return want
    assert chain_case("honest chain", segs, True, [], [144], halt, False) == 0
    for k, (ins, outs, hk) in enumerate(claims):
        assert chain_case(f"chain claim{k}", segs, bool(k & 1), ins, outs, hk, True) != 0
    for i, (label, chain) in enumerate(_chain_mutants(segs, rng, 200)):
        chain_case(label, chain, i % 2 == 0 or _is_prefix(chain, segs), [], [144], halt, True)
    assert len(c.cases) >= 450
    _check(driver, c, min_codes=4)
    print(f"io: {len(c.cases)} cases")


# ---- low-degree proofs -----------------------------------------------------------------------------------------------------------------------------------------------------
def _lowdeg_mutants(proof, rng):
    at = LD.layout(proof)
    n = len(proof)
    out = []

    def put(label, pos, val):
        t = proof.copy(); t[pos] = val & 0xFFFFFFFF
        out.append((label, t))
    for pos in range(8):                                            # magic, version, log_n, b, width, num_queries, pow_bits, n_layers
        for v in EDGES + [int(proof[pos]) + 1, max(int(proof[pos]) - 1, 0), 2, 3, 4, 24, 25, 26, 27, 128, 129, 512, 513]:
            put(f"header{pos}={v}", pos, v)
    starts = [at["queries"] + t * at["qsize"] for t in range(at["num_queries"])]
    for s in starts:                                                # the query index words
        for v in EDGES + [int(proof[s]) ^ 1, int(proof[s]) + (1 << (at["log_n"] + at["b"] - 1))]:
            put(f"query@{s}={v}", s, v)
    bounds = [8, 12, at["final"], at["nonce"], at["queries"]] + starts + [starts[0] + 1 + at["rec"], starts[0] + at["layers"][0][0], starts[0] + at["layers"][0][1], n]
    for b in bounds:
        for cut in (b - 1, b, b + 1):
            if 0 <= cut <= n:
                out.append((f"cut{cut}", proof[:cut].copy()))
    for cut in rng.integers(0, n, 12):
        out.append((f"cut{cut}", proof[:int(cut)].copy()))
    for extra in (1, 3, 32):
        out.append((f"extend{extra}", np.concatenate([proof, rng.integers(0, P, extra).astype(np.uint32)])))
    for pos in [8, 12, at["final"], at["final"] + 4 * at["n_fin"] - 1, at["nonce"], starts[0] + 1, starts[0] + at["layers"][0][0], starts[0] + at["layers"][0][1], starts[-1] + at["layers"][-1][0],
                starts[-1] + at["layers"][-1][1], n - 1] + [int(x) for x in rng.integers(12, n, 30)]:
        put(f"word{pos}+1", pos, (int(proof[pos]) + 1) % P)
    for pos in rng.integers(0, n, 8):
        put(f"word{pos}>=p", int(pos), [P, P + 1, 0xFFFFFFFF][int(pos) % 3])
    for _ in range(10):
        a, b = (int(x) for x in rng.integers(8, n, 2))
        t = proof.copy(); t[a], t[b] = t[b], t[a]
        out.append((f"swap{a},{b}", t))
        a = int(rng.integers(8, n))
        t = proof.copy(); t[a:a + int(rng.integers(1, 40))] = 0
        out.append((f"zero{a}", t))
    return [(label, t) for label, t in out if not _same(t, proof)]


def test_lowdeg_verify(driver):
    """zkir_lowdeg_verify, with and without `expect_root`, on three reference proofs with distinct schedules and about 500 mutants of them."""
    c = Corpus("lowdeg")
    rng = np.random.default_rng(4400)
    assert len({tuple(LD.schedule(log_n, b)) for log_n, b in ((3, 1), (5, 2), (6, 3))}) == 3
    for log_n, b, width, nq, pow_bits in ((3, 1, 3, 3, 2), (5, 2, 5, 4, 3), (6, 3, 9, 3, 4)):
        cols = np.stack([so.lde(rng.integers(0, P, 1 << log_n).astype(np.uint32), b)[1] for _ in range(width)])
        proof = LD.prove_ref(cols, b, nq, pow_bits)
        root = proof[8:12].copy()
        wrong_root = root.copy(); wrong_root[2] ^= 1
        assert LD.verify_ref(proof, root) == 0
        base = c.base(proof)
        c.add("honest", LOWDEG, [0], [(base, proof)], "rc 0")
        c.add("honest, its root", LOWDEG, [1], [(base, proof), root], "rc 0")
        c.add("honest, another root", LOWDEG, [1], [(base, proof), wrong_root], "rc 2", mutant=True, accepted=False)
        for i, (label, t) in enumerate(_lowdeg_mutants(proof, rng)):
            expect = [None, root, wrong_root][i % 3] if i % 7 else root
            want = LD.verify_ref(t, expect)
            c.add(f"log_n {log_n} {label}", LOWDEG, [int(expect is not None)], [(base, t)] + ([expect] if expect is not None else []), f"rc {want}", mutant=True, accepted=want == 0)
    assert len(c.cases) >= 450
    _check(driver, c, min_codes=4)
    print(f"lowdeg: {len(c.cases)} cases")


# ---- opening records -------------------------------------------------------------------------------------------------------------------------------------------------------
def test_merkle_verify_host(driver):
    """zkir_merkle_verify_host, row form and digest form: merkle_open_ref's records and mutations, refused arguments, an empty batch, a tree of one leaf."""
    c = Corpus("merkle")
    rng = np.random.default_rng(4500)

    def case(label, root, width, n_leaves, indices, records, flags, mutant=False):
        indices, records = np.asarray(indices, np.uint64), np.asarray(records, np.uint32).reshape(-1)
        refused = n_leaves == 0 or n_leaves & (n_leaves - 1) or (flags & MO.LEAF_DIGEST and width != 0)
        if refused:
            want, ok = "error 9", False
        else:
            assert len(records) == len(indices) * MO.record_words(width, n_leaves, flags)
            v, s = MO.verify_all_ref(root, width, n_leaves, indices, records, flags)
            want, ok = f"summary {s[0]} {s[1]} verdicts" + "".join(f" {x}" for x in v), not s[0]
        c.add(label, MERKLE, [width, n_leaves, flags], [np.asarray(root, np.uint32), indices, records], want, mutant=mutant, accepted=ok if mutant else None)
    for width, n in ((5, 16), (8, 1), (1, 2), (13, 64)):
        cols = rng.integers(0, P, (width, n)).astype(np.uint32)
        root, layers = so.merkle(cols, want_layers=True)
        idx = list(range(n)) if n <= 16 else [int(x) for x in rng.integers(0, n, 24)]
        rows = np.stack([MO.open_ref(cols, layers, i) for i in idx])
        digests = np.stack([MO.open_ref(None, layers, i) for i in idx])
        case(f"rows {width}x{n}", root, width, n, idx, rows, 0)
        case(f"digests {n}", root, 0, n, idx, digests, MO.LEAF_DIGEST)
        case(f"empty batch {n}", root, width, n, [], [], 0)
        for seed in range(3):
            case(f"rows {width}x{n} mutated {seed}", root, width, n, *MO.mutations(width, n, idx, rows, 0, seed), 0, mutant=len(idx) >= 8)
            case(f"digests {n} mutated {seed}", root, 0, n, *MO.mutations(0, n, idx, digests, MO.LEAF_DIGEST, seed), MO.LEAF_DIGEST, mutant=len(idx) >= 8)
        bad_root = root.copy(); bad_root[0] = (int(bad_root[0]) + 1) % P
        case(f"another root {n}", bad_root, width, n, idx, rows, 0, mutant=True)
        for n_bad in (0, 3, 6, (1 << 63) + 1, U64_MAX):               # refused before a record is read
            case(f"n_leaves {n_bad}", root, width, n_bad, idx, rows, 0, mutant=True)
        case("digest form with a width", root, width, n, idx, digests, MO.LEAF_DIGEST, mutant=True)
        # the same records against a tree claimed twice / half as deep: a record is as long as the claim says
        for n_claim in (2 * n, n // 2):
            if n_claim >= 1:
                words = MO.record_words(width, n_claim)
                padded = np.zeros((len(idx), words), np.uint32)
                padded[:, :min(words, rows.shape[1])] = rows[:, :words]
                case(f"rows {width}x{n} as {n_claim} leaves", root, width, n_claim, idx, padded, 0, mutant=n_claim > 1)
    _check(driver, c)
    # This entry point has one refusal code (error 9: n_leaves or the form's width); everything else it reports per record.  So the family's spread is asserted over the
    # ways its mutants are turned down: the refusal, and the record verdicts 1 (another root), 2 (a word >= p), 3 (an index >= n_leaves) — four values, each of them met.
    ways = set()
    for x in c.cases:
        if x["mutant"]:
            ways |= {"error 9"} if x["want"] == "error 9" else {int(v) for v in x["want"].split(" verdicts")[1].split()} - {0}
    assert ways == {"error 9", 1, 2, 3}, ways
    print(f"merkle: {len(c.cases)} cases")


# ---- the tapes of mode 4 ---------------------------------------------------------------------------------------------------------------------------------------------------
def _tape_words_used(words):
    q = 1
    for _ in range(int(words[0])):
        q += 8 + 5 * int(words[q + 7])
    return q


def _section_digests_crc(hash_words, wide_words):
    dg = []
    for sec in (hash_words, wide_words):
        dg += [so.hash_elems(sec[k:k + 512]) for k in range(0, len(sec), 512)]
    return zlib.crc32(np.concatenate(dg).astype("<u4").tobytes())


def test_tape_stages_and_hash_helpers(driver):
    """hashcall::parse_section (what zkir_hash_tape_check_host forwards to), the verifier's host tape stages (the sum that zkir_tape_table_side_host forms by other code, not
    that function's body; the sections' chunk digests), hashcall::new_bytes (zkir_hash_tape_new_bytes_host's per-call function, without its threaded copy),
    zkir_hash_call_cells_host and zkir_digest_bytes on the designed sections of the tape references, malformed ones included."""
    c = Corpus("tapes")
    rng = np.random.default_rng(4600)
    base_words, at = TS.check_tape()
    b = c.base(base_words)

    def check_case(label, words, n_real=TS.CHECK_N_REAL, code_end=TS.CHECK_CODE_END, mutant=False):
        code = TS.expected_check_code(words, n_real, code_end)
        want = f"code 0 used {_tape_words_used(words)}" if code == 0 else f"code {code}"
        c.add(label, HASH_CHECK, [n_real, code_end], [(b, np.asarray(words, np.uint32))], want, mutant=mutant, accepted=(code == 0) if mutant else None)
    check_case("the three-call tape", base_words)
    check_case("the empty section", TS.EMPTY)
    check_case("no words", np.zeros(0, np.uint32))
    for name, words in TS.check_mutations():
        check_case(name, words, mutant=True)
    for pos in range(len(base_words)):                              # every word of the tape at the edges (a third of them each, round-robin)
        for v in EDGES[pos % 3::3] + [int(base_words[pos]) + 1]:
            t = base_words.copy(); t[pos] = v & 0xFFFFFFFF
            if not _same(t, base_words):
                check_case(f"word{pos}={v}", t)
    for cut in range(0, len(base_words), 3):
        check_case(f"cut{cut}", base_words[:cut], mutant=True)
    check_case("longer than its records", np.concatenate([base_words, [0, 0]]))
    check_case("no row bound, no code", base_words, n_real=U64_MAX, code_end=0)
    check_case("code up to 2^40", base_words, code_end=1 << 40)
    for name in ("designed",):
        check_case(name, TD.tape(name), n_real=1 << 20, code_end=0x1000)

    alpha, lam = np.array(TS.ALPHA, np.uint32), np.array(TS.LAM, np.uint32)

    def side_case(label, hw, ww, a=alpha, l=lam, want=None):
        if want is None:
            ref = TS.reference(hw if len(hw) else TS.EMPTY, TD.expected_new_bytes(hw) if len(hw) else np.zeros(0, np.uint64), ww if len(ww) else TS.EMPTY)
            want = "sum " + " ".join(str(int(x)) for x in ref["sum"]) + f" digests {_section_digests_crc(hw if len(hw) else TS.EMPTY, ww if len(ww) else TS.EMPTY):08x}"
        c.add(label, TAPE_SIDE, [], [np.asarray(hw, np.uint32), np.asarray(ww, np.uint32), a, l], want)
    for name in ("empty", "len0", "spans", "items255", "items256", "items257", "wide_sorted", "wide_reversed", "wide_blocks", "both"):
        hw, _, ww = TS.synthetic(name)
        side_case(name, hw, ww, want="refused 57" if name == "wide_reversed" else None)      # (the verifier's record check wants the wide tape in cycle order)
    side_case("no sections at all", np.zeros(0, np.uint32), np.zeros(0, np.uint32))
    hw, _, ww = TS.synthetic("both")
    for name, words in TS.check_mutations():
        code = TS.expected_check_code(words, U64_MAX, 0)
        if code or _tape_words_used(words) != len(words):
            side_case("malformed hash tape " + name, words, ww, want=f"refused {code or 4}")
    side_case("wide count above its words", hw, np.concatenate([[len(ww)], ww[1:]]).astype(np.uint32), want="refused wide")
    side_case("wide section cut", hw, ww[:-1], want="refused wide")
    for label, pos, v in (("opcode 8", 8, 8), ("opcode 2", 8, 2), ("a limb of 2^20", 2, 1 << 20), ("a high limb of 2^24", 4, 1 << 24), ("records out of order", 9, 0)):
        t = ww.copy(); t[pos] = v
        side_case("wide " + label, hw, t, want="refused 57")
    t = ww.copy(); t[1 + 8 + 4:1 + 8 + 7] = 0                       # DIVU by zero: never a row
    side_case("wide zero divisor", hw, t, want="refused 57")
    bad = alpha.copy(); bad[3] = P
    side_case("alpha not canonical", hw, ww, a=bad, want="refused challenge")
    side_case("lambda not canonical", hw, ww, l=np.array([0, 0, 0xFFFFFFFF, 0], np.uint32), want="refused challenge")

    def bytes_case(label, words, no_out=False):
        """no_out: the caller hands no array for the bytes (refused where the section has cells; asked only after the section parsed)"""
        code = TS.expected_check_code(words, U64_MAX, 0) if len(words) else 0
        if code or (len(words) and _tape_words_used(words) != len(words)):
            want = f"refused {code or 4}"
        else:
            nb = TD.expected_new_bytes(words if len(words) else TS.EMPTY)
            want = "refused null" if no_out and len(nb) else f"cells {len(nb)} crc {zlib.crc32(nb.astype('<u8').tobytes()):08x}"
        c.add(label, NEW_BYTES, [int(no_out)], [np.asarray(words, np.uint32)], want)
    for name in ("designed", "l_dev"):
        bytes_case("new bytes " + name, TD.tape(name))
    # regression: a call of length 0 hashed an empty vector's null data pointer through memcpy (undefined even for 0 bytes) in sha256 / keccak256 / blake3
    bytes_case("regression: calls of length 0, every kind", TS.make_tape([(4, 0x2000, 0, 0x3000, 3), (5, 0x2001, 0, 0x3041, 5), (6, 0x2002, 0, 0x3087, 6)], seed=2)[0])
    bytes_case("new bytes of the three-call tape", base_words)
    bytes_case("new bytes of nothing", np.zeros(0, np.uint32))
    bytes_case("new bytes of the three-call tape, no array", base_words, no_out=True)
    bytes_case("new bytes of nothing, no array", np.zeros(0, np.uint32), no_out=True)
    bytes_case("new bytes of no calls, no array", TS.EMPTY, no_out=True)
    bytes_case("new bytes of a cut tape, no array", base_words[:-1], no_out=True)
    for name, words in TS.check_mutations():
        bytes_case("new bytes " + name, words)

    calls = [(cc[1], cc[2], cc[3], cc[4]) for cc in TD.designed_calls()]
    calls += [(0x2000, (1 << 20) + 1, 0x3000, 5), (0x2000, 8, 0x3002, 3), (0x2000, 8, 0x3000, 4), (1 << 40, 0, 0x3000, 5), ((1 << 40) - 8, 9, 0x3000, 6), (0x2000, 8, (1 << 40) - 31, 6),
              (U64_MAX, 1, 0x3000, 5), (0x2000, U64_MAX, 0x3000, 5), (0x2000, 8, U64_MAX - 3, 3), (U64_MAX - 7, 8, U64_MAX - 31, 5)]
    for in_ptr, length, out_ptr, kind in calls:
        ok = kind in (3, 5, 6) and (kind != 3 or out_ptr % 4 == 0) and length <= 1 << 20 and in_ptr < 1 << 40 and in_ptr + length <= 1 << 40 and out_ptr < 1 << 40 and out_ptr + 32 <= 1 << 40
        cells = TS.cells_of(in_ptr, length, out_ptr) if ok else []
        probes = ([cells[0], cells[-1], cells[len(cells) // 2], cells[0] + 1, cells[-1] + 8, max(cells[0] - 8, 0)] if ok else [0, 0x3000]) + [U64_MAX, U64_MAX - 7]
        for cell in probes:
            want = f"cells {len(cells)} rank {cells.index(cell) if cell in cells else U64_MAX}" if ok else f"cells {U64_MAX} rank {U64_MAX}"
            c.add(f"cells of {in_ptr:#x}+{length} -> {out_ptr:#x} kind {kind} at {cell:#x}", CALL_CELLS, [in_ptr, length, out_ptr, kind, cell], [], want)

    for n in [0, 1, 2, 3, 15, 16, 17, 1023, 1024, 1025, 4095] + [int(x) for x in rng.integers(0, 3000, 10)]:
        data = rng.integers(0, 256, n).astype(np.uint8)
        c.add(f"digest of {n} bytes", DIGEST_BYTES, [], [data], "digest " + " ".join(str(int(x)) for x in so.digest_bytes(data.tobytes())))
    _check(driver, c)
    # hashcall::parse_section has three codes only (4 cut short, 55 an output over the code, 56 a bad record), so the family's spread is taken over every refusal of its
    # entry points: those three from the hash-tape check (direct, and as "refused" by the two that parse first), 57 from the wide tape's record check, the refused arguments
    turned_down = {w.split()[1] for w in (x["want"] for x in c.cases) if w.startswith("refused ") or (w.startswith("code ") and not w.startswith("code 0"))}
    assert turned_down >= {"4", "55", "56", "57", "wide", "challenge"}, turned_down
    for kind in (HASH_CHECK, TAPE_SIDE, NEW_BYTES):                 # and none of the three collapses into one exit
        assert len({x["want"].split()[1] for x in c.cases if x["kind"] == kind and x["want"].split()[0] in ("refused", "code") and not x["want"].startswith("code 0")}) >= 3, kind
    print(f"tapes: {len(c.cases)} cases")


# ---- program blobs and the interpreter -------------------------------------------------------------------------------------------------------------------------------------
CONFIGS = [dict(), dict(enable_range_checking=True), dict(enable_deferred_model=True), dict(enable_range_checking=True, enable_deferred_model=True),
           dict(enable_execution_trace=True), dict(enable_execution_trace=True, enable_range_checking=True), dict(enable_execution_trace=True, enable_deferred_model=True)]
MAX_CYCLES = 2000


def _blob_mutants(blob, rng, n):
    out = []
    code_size = int.from_bytes(blob[16:20], "little") if len(blob) >= 20 else 0
    for it in range(n):
        t = bytearray(blob)
        kind = it % 6
        if kind == 0 and len(t) >= 32:                              # a header field at an edge
            off = [0, 4, 12, 16, 20, 24, 28][int(rng.integers(0, 7))]
            t[off:off + 4] = int(EDGES[int(rng.integers(0, len(EDGES)))]).to_bytes(4, "little")
        elif kind == 1 and len(t) >= 32:                            # a configuration byte; code_size at / around / past the blob's end
            if rng.integers(0, 2):
                t[8 + int(rng.integers(0, 4))] = int(rng.integers(0, 256))
            else:
                t[16:20] = max(len(t) - 32 + int(rng.integers(-8, 9)), 0).to_bytes(4, "little")
        elif kind in (2, 3) and code_size >= 4 and len(t) >= 32 + code_size:      # random instruction words: any 32 bits, or another opcode under the same fields
            for _ in range(int(rng.integers(1, 4))):
                at = 32 + 4 * int(rng.integers(0, code_size // 4))
                word = int(rng.integers(0, 1 << 32)) if kind == 2 else (int.from_bytes(t[at:at + 4], "little") & ~0x7F) | int(rng.integers(0, 128))
                t[at:at + 4] = word.to_bytes(4, "little")
        elif kind == 4:                                             # truncations, below 32 bytes among them
            t = t[:int(rng.integers(0, 40)) if rng.integers(0, 2) else int(rng.integers(0, len(t) + 1))]
        else:                                                       # data_size / entry point around the blob; bytes appended
            if len(t) >= 32 and rng.integers(0, 2):
                t[20:24] = max(len(t) - 32 - code_size + int(rng.integers(-4, 5)), 0).to_bytes(4, "little")
            else:
                t += bytes(rng.integers(0, 256, int(rng.integers(1, 16))).astype(np.uint8))
        if bytes(t) != blob:
            out.append((f"{it}/{kind}", bytes(t)))
    return out


def _interp_want(blob, ins, cfg):
    try:
        res = oracle.run(blob, list(ins), want_sorted=False, **cfg)
    except oracle.OracleError:
        return "error", None
    outs = np.asarray(res.outputs, "<u8")
    return f"halt {res.halt_kind} {res.halt_code if res.halt_kind == 1 else 0} cycles {res.cycles} outputs {len(outs)} {zlib.crc32(outs.tobytes()):08x}", res


def test_interpreter_and_memory_witness_on_damaged_blobs(driver):
    """zkir::interpret (what zkir_interpret forwards to) under every configuration, and zkir_memcheck_witness_of_mode on the traced logs, on the programs of tests/programs.py
    and about 2000 damaged copies, at most 2000 cycles each: refused or accepted as by oracle.run, and an accepted run's halt kind, halt code, cycle count and outputs."""
    c = Corpus("blobs")
    rng = np.random.default_rng(4700)
    progs = [(name, *f()[:3]) for name, f in pg.ALL.items()] + [(name, *f()[:3]) for name, f in pg.ERRORS.items()]
    progs += [(name, *f()[:3]) for name, f in list(pg.MEM_EDGES.items()) + list(pg.MEM_EDGES_NO_PROOF.items()) + list(pg.HASH_EDGES.items()) + list(pg.HASH_EDGES_NO_PROOF.items())]
    # regression: hash_edge_max_len (above) is the one program here whose traced log outgrows 8 MiB and so parks blocks in the interpreter's pool (interp.cpp); the pool's
    # vector was destroyed at exit with the blocks still in it, which LeakSanitizer reports as a direct leak
    progs.append(("wide_and_hash", *TS.wide_and_hash_program()))
    progs.append(("random7", *pg.random_program(7, n_instr=120), {}))
    # regression: a traced SHA-256 syscall over zero bytes copied from an empty vector's null data pointer into the SHA block record (interp.cpp, undefined even for 0 bytes)
    progs.append(("regression_sha256_of_nothing", pg._p([pg.A(11, 0, 0x2000), pg.A(12, 0, 0), pg.A(13, 0, 0x3000), pg.A(10, 0, 3), pg.EC] + pg._exit0()), [], {}))

    no_witness = set(pg.MEM_EDGES_NO_PROOF) | set(pg.HASH_EDGES_NO_PROOF) | set(pg.ERRORS)

    def case(label, blob, ins, cfg, witness_mode, mutant_of=None):
        want, res = _interp_want(blob, ins, cfg)
        args = [cfg["max_cycles"], cfg.get("enable_range_checking", 0), cfg.get("enable_execution_trace", 0), cfg.get("enable_deferred_model", 0), witness_mode]
        if res is not None and witness_mode and mutant_of is None and res.halt_kind != 2 and label.split()[0] not in no_witness and not (len(res.memops) and int(res.memops["address"].max()) >> 40):      # (an access at 2^40 or above has no witness)
            # an honest traced run: the witness's touched cells and hash calls are the oracle's
            pub = so.public_inputs(len(res.rows), blob, list(ins), list(res.outputs), (res.halt_kind, res.halt_code), wide_mode=True)
            n_calls = int(so.hash_section(res.rows, pub)[0])
            if witness_mode == 4 or n_calls == 0:
                want += f" witness cells {len(so.mem_cells(res.rows, pub))} accesses"
        c.add(label, INTERPRET, args, [np.frombuffer(blob, np.uint8) if mutant_of is None else (mutant_of, np.frombuffer(blob, np.uint8)), np.asarray(list(ins), np.uint64)], want)
    per_prog = max(2000 // len(progs), 1)
    for k, (name, blob, ins, cfg) in enumerate(progs):
        cycles = min(cfg.get("max_cycles", MAX_CYCLES), MAX_CYCLES)
        base = c.base(np.frombuffer(blob, np.uint8))
        for j, conf in enumerate(CONFIGS):
            traced = conf.get("enable_execution_trace") and not conf.get("enable_deferred_model")
            case(f"{name} {conf}", blob, ins, dict(conf, max_cycles=cycles), (3 + j % 2) if traced else 0)
        for j, (label, t) in enumerate(_blob_mutants(blob, rng, per_prog)):
            conf = CONFIGS[(j + k) % len(CONFIGS)]
            traced = conf.get("enable_execution_trace") and not conf.get("enable_deferred_model")
            case(f"{name} {label}", t, ins, dict(conf, max_cycles=cycles), (3 + j % 2) if traced else 0, mutant_of=base)
    # every header field of one program at every edge, every configuration byte at the ends of its range and beyond
    name, blob, ins, _ = progs[[x[0] for x in progs].index("fib30")]
    base = c.base(np.frombuffer(blob, np.uint8))
    grid = [(off, 4, v) for off in (0, 4, 12, 16, 20, 24, 28) for v in EDGES + [len(blob) - 32, len(blob) - 31, len(blob) - 28]]
    grid += [(off, 1, v) for off in (8, 9, 10, 11) for v in (0, 1, 2, 3, 4, 5, 15, 16, 17, 20, 29, 30, 31, 32, 255)]
    for j, (off, size, v) in enumerate(grid):
        t = bytearray(blob); t[off:off + size] = int(v).to_bytes(size, "little")
        conf = CONFIGS[j % len(CONFIGS)]
        case(f"{name} header byte {off} = {v}", bytes(t), ins, dict(conf, max_cycles=MAX_CYCLES), 3 if conf == CONFIGS[4] else 0, mutant_of=base)
    assert len(c.cases) >= 1800
    # oracle.run gives a refused blob no code, so this family's spread is not counted in rejection codes: a quarter of the cases at least must run, and end in every halt kind
    ran = [x["want"] for x in c.cases if x["want"].startswith("halt")]
    assert 4 * len(ran) >= len(c.cases) and len({w.split()[1] for w in ran}) == 3, "the damaged blobs collapse into refusals"
    _check(driver, c)
    print(f"blobs: {len(c.cases)} cases over {len(progs)} programs")


def test_the_restated_padded_log_n_is_the_librarys(driver):
    """The driver restates zkir_padded_log_n (the library defines it beside its kernels): equal for n = 1 .. 2^12 and at 2^k - 1, 2^k, 2^k + 1 up to 2^26."""
    from zkir_amd import runtime as rt
    ns = list(range(1, (1 << 12) + 1)) + [(1 << k) + d for k in range(1, 27) for d in (-1, 0, 1)]
    c = Corpus("log_n")
    c.add("padded_log_n", PADDED_LOG_N, [], [np.array(ns, np.uint64)], "log_n" + "".join(f" {int(rt.lib().zkir_padded_log_n(n))}" for n in ns))
    _check(driver, c)
