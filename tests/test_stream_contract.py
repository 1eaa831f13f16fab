"""The stream contract of every device entry point (include/gcsa2_hip.h): work is enqueued on the CALLER's stream -- "only
enqueue work on `stream`" or "enqueued on `stream`, complete on return" -- and one handle serves several host threads, each on
a stream of its own.  tests/streams.py has the probes: the real batch reaches the input buffers on the caller's stream behind
a delay (until then they hold a decoy batch of the same offsets and shapes), and the legacy default stream is kept busy while
the caller's stream is free.  Only the caller's stream is waited for.  The expectation of a case is the same call on the
default stream between two device-wide waits, made here and pinned against the oracle by the feature tests; find, count,
parent, locate_into and match_stats are compared with the oracle here as well.

Shapes: the 6000-base SNP graph with the reads of the k-mer tests, k = 8 and 16, hit_max = 3 with sampling (the "over" paths
run); for locate the index of test_locate_segment_sizes with one range per size class."""
import ctypes
import functools
import os
import re
import threading

import numpy as np
import pytest

import streams
from streams import Case, ENQUEUE, ONE_WAIT, COMPLETE
from gcsa2_amd.hostview import concat_patterns, pack_kmers
from test_extend import GRAPHS, BIG, indexed, batch
from test_kmer_windows import reads_of, walks, window_count
from test_seed_clusters import synthetic, identity_map

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIT_MAX, SAMPLE = 3, 1
SHIFT = 11                                                # value >> 11 = node id (support.h:443-471)


# ---- the table ---------------------------------------------------------------------------------------------------------
# One row per binding method (or per form of one): the C entry point it reaches and its contract class, in the header's words.
TABLE = {
    "find_device":                  ("gcsa2_find_device", ENQUEUE),
    "find_packed_device":           ("gcsa2_find_packed_device", ENQUEUE),
    "find_stats_device":            ("gcsa2_find_stats_device", ENQUEUE),
    "find_device_variant-2":        ("gcsa2_find_device_variant", ENQUEUE),
    "find_device_variant-4":        ("gcsa2_find_device_variant", ENQUEUE),
    "lf_device":                    ("gcsa2_lf_device", ENQUEUE),
    "count_device":                 ("gcsa2_count_device", ENQUEUE),
    "parent_device":                ("gcsa2_parent_device", ENQUEUE),
    "extend_device":                ("gcsa2_extend_device", ENQUEUE),
    "kmer_windows_device":          ("gcsa2_kmer_windows_device", COMPLETE),
    "kmer_hits_device":             ("gcsa2_kmer_hits_device", COMPLETE),
    "minimizers_device":            ("gcsa2_minimizers_device", COMPLETE),
    "minimizer_hits_device":        ("gcsa2_minimizer_hits_device", COMPLETE),
    "capped_seeds_device":          ("gcsa2_capped_seeds_device", COMPLETE),
    "kmer_support_device":          ("gcsa2_kmer_support_device", COMPLETE),
    "seed_support_device":          ("gcsa2_seed_support_device", COMPLETE),
    "index_kmer_support_device":    ("gcsa2_index_kmer_support_device", COMPLETE),
    "kmer_classes_device":          ("gcsa2_kmer_classes_device", COMPLETE),
    "seed_classes_device":          ("gcsa2_seed_classes_device", COMPLETE),
    "kmer_top_classes_device":      ("gcsa2_kmer_top_classes_device", COMPLETE),
    "seed_top_classes_device":      ("gcsa2_seed_top_classes_device", COMPLETE),
    "seed_clusters_device":         ("gcsa2_seed_clusters_device", COMPLETE),
    "seed_clusters_device-lds64":   ("gcsa2_seed_clusters_device", COMPLETE),
    "kmer_clusters_device":         ("gcsa2_kmer_clusters_device", COMPLETE),
    "minimizer_clusters_device":    ("gcsa2_minimizer_clusters_device", COMPLETE),
    "match_stats_device-0":         ("gcsa2_match_stats_device_variant", ONE_WAIT),    # "ONE wait for `stream` per call"
    "match_stats_device-2":         ("gcsa2_match_stats_device_variant", ONE_WAIT),
    "match_stats_device-5-sized":   ("gcsa2_match_stats_device_sized", ENQUEUE),
    "match_breaks_device":          ("gcsa2_match_breaks_bounded_device", COMPLETE),
    "match_breaks_device-bounded":  ("gcsa2_match_breaks_bounded_device", COMPLETE),
    "match_stats_profile_device":   ("gcsa2_match_stats_profile_device", ENQUEUE),
    "mem_hits_device":              ("gcsa2_mem_hits_bounded_device", COMPLETE),
    "mem_hits_device-bounded":      ("gcsa2_mem_hits_bounded_device", COMPLETE),
    "sub_mem_hits_device":          ("gcsa2_sub_mem_hits_device", COMPLETE),
    "locate_device":                ("gcsa2_locate_device", COMPLETE),
    "locate_into-sorted":           ("gcsa2_locate_into", COMPLETE),
    "locate_into-unsorted":         ("gcsa2_locate_into", COMPLETE),
    "locate_max_into":              ("gcsa2_locate_max_into", COMPLETE),
    "pack_ranges32_device":         ("gcsa2_pack_ranges32_device", ENQUEUE),
    "unpack_ranges32_device":       ("gcsa2_unpack_ranges32_device", ENQUEUE),
    "pack_ranges40_device":         ("gcsa2_pack_ranges40_device", ENQUEUE),
    "unpack_ranges40_device":       ("gcsa2_unpack_ranges40_device", ENQUEUE),
    "pack_ranges48_device":         ("gcsa2_pack_ranges48_device", ENQUEUE),
    "unpack_ranges48_device":       ("gcsa2_unpack_ranges48_device", ENQUEUE),
}

# Declarations with a `void* stream` that have no row, each with its reason.
EXCLUDED = {
    "gcsa2_match_stats_device": "gcsa2_match_stats_device_variant with variant 0, which has a row (the binding reaches it through that form)",
    "gcsa2_match_breaks_device": "gcsa2_match_breaks_bounded_device with max_length 0, which has a row (the binding reaches it through that form)",
    "gcsa2_mem_hits_device": "gcsa2_mem_hits_bounded_device with max_length 0, which has a row (the binding reaches it through that form)",
    "gcsa2_comm_gather": "a collective: needs several ranks",
    "gcsa2_comm_match_stats": "a collective: needs several ranks",
    "gcsa2_comm_locate": "a collective: needs several ranks",
    "gcsa2_gather_fn": "a callback type of the caller, not an entry point",
}
# (The gcsa2_group_* forms take no stream: they own one per replica.)


def declarations_with_a_stream(text):
    """The names of the declarations of the header that take a `void* stream`: functions and function-pointer types."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    names = set()
    for statement in text.split(";"):
        if not re.search(r"void\s*\*\s*stream\s*\)\s*$", statement.strip()):
            continue
        found = re.findall(r"\b(gcsa2_\w+)\s*\)?\s*\(", statement)          # `name(` or `(*name)(`
        assert found, statement
        names.add(found[0])
    return names


def test_every_stream_entry_point_has_a_row():
    """A declaration of include/gcsa2_hip.h with a `void* stream` parameter has a row in TABLE or a reason in EXCLUDED: a new
    entry point cannot skip the contract test.  Every row names a declaration, and every row's binding method exists."""
    with open(os.path.join(ROOT, "include", "gcsa2_hip.h")) as f:
        declared = declarations_with_a_stream(f.read())
    assert len(declared) > 40 and "gcsa2_find_device" in declared and "gcsa2_unpack_ranges48_device" in declared and "gcsa2_gather_fn" in declared
    rows = {c for c, _ in TABLE.values()}
    assert not (rows - declared), sorted(rows - declared)
    assert not (set(EXCLUDED) - declared), sorted(set(EXCLUDED) - declared)
    assert not (rows & set(EXCLUDED)), sorted(rows & set(EXCLUDED))
    missing = declared - rows - set(EXCLUDED)
    assert not missing, ("no row in TABLE and no reason in EXCLUDED", sorted(missing))
    assert all(reason for reason in EXCLUDED.values())
    from gcsa2_amd import binding
    for row in TABLE:
        method = row.split("-")[0]
        assert hasattr(binding.GCSA, method) or hasattr(binding, method), row
    assert set(TABLE) == set(BUILDERS), sorted(set(TABLE) ^ set(BUILDERS))


# ---- the batches ---------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def read_batches():
    """(real, decoy): the reads of the k-mer tests on the 6000-base graph, and other walks through it cut to the same lengths."""
    real = reads_of(BIG)
    spare = walks(GRAPHS[BIG][1], 0xDEC0, len(real), lo=63, hi=63)
    assert max(len(r) for r in real) <= 63
    decoy = [spare[q][:len(r)] for q, r in enumerate(real)]
    assert [len(r) for r in real] == [len(r) for r in decoy] and sum(a != b for a, b in zip(real, decoy)) > len(real) // 2
    return real, decoy


def reads_input(pair=None):
    """The inputs `pat` and `off` of a read batch: the bytes differ, the offsets are shared."""
    real, decoy = pair or read_batches()
    (d0, off), (d1, off1) = concat_patterns(real), concat_patterns(decoy)
    assert np.array_equal(off, off1)
    total = int(off[-1])
    return {"pat": (d0[:total], d1[:total]), "off": (off, off)}, len(real), total


def u64(a):
    return np.ascontiguousarray(a, dtype=np.uint64)


def words(raw, key, shape=-1):
    return raw[key].view(np.uint64).reshape(shape)


class Env:
    """What the builders share: the handles, the oracles and a few derived batches (made once)."""

    def __init__(self, engine, gpu, seg_gpu, seg_cpu, seg_n):
        self.engine, self.gpu, self.cpu = engine, gpu, indexed(BIG)[1]
        self.seg_gpu, self.seg_cpu, self.seg_n = seg_gpu, seg_cpu, seg_n
        self.cache = {}

    def flat(self, which):
        reads = read_batches()[which]
        return concat_patterns(reads)

    def found_ranges(self):
        """(real, decoy): the non-empty find() ranges of the 8-mers at stride 5 of either batch, cut to one length -- valid
        search states, not the same ones."""
        if "found" not in self.cache:
            out = []
            for which in (0, 1):
                wins = [r[j:j + 8] for r in read_batches()[which] for j in range(0, max(len(r) - 7, 0), 5)]
                rng = self.cpu.find_batch(*concat_patterns(wins))
                out.append(rng[(rng[:, 0] + np.uint64(1)) <= (rng[:, 1] + np.uint64(1))])
            m = min(out[0].shape[0], out[1].shape[0], 3000)
            assert m > 500
            self.cache["found"] = (out[0][:m].copy(), out[1][:m].copy())
        return self.cache["found"]

    def all_ranges(self):
        """(real, decoy): find() of every read's 8-mers at stride 5, the empty ranges (both forms) included."""
        if "all" not in self.cache:
            out = []
            for which in (0, 1):
                wins = [r[j:j + 8] for r in read_batches()[which] for j in range(0, max(len(r) - 7, 0), 5)]
                out.append(self.cpu.find_batch(*concat_patterns(wins)))
            self.cache["all"] = tuple(out)
        return self.cache["all"]

    def seeds(self):
        """(real, decoy): the seed records of the 8-mers of either batch (the host form), cut to one number of records."""
        if "seeds" not in self.cache:
            out = [self.gpu.kmer_hits_batch(*self.flat(which), 8, 1, HIT_MAX, True)[1] for which in (0, 1)]
            m = min(out[0].shape[0], out[1].shape[0], 4000)
            assert m > 500
            self.cache["seeds"] = (u64(out[0][:m]), u64(out[1][:m]))
        return self.cache["seeds"]

    def n_bins(self):
        if "bins" not in self.cache:
            self.cache["bins"] = (int(np.asarray(self.cpu.locate((0, self.cpu.n - 1)), dtype=np.uint64).max()) >> SHIFT) + 1
        return self.cache["bins"]


def sized(*sizes):
    """The capacity that holds the real and the decoy batch."""
    return max(int(s) for s in sizes) + 1


# ---- builders: name -> Case ------------------------------------------------------------------------------------------------

BUILDERS = {}


def row(name):
    def register(f):
        BUILDERS[name] = f
        return f
    return register


def find_oracle(env):
    def check(out, result):
        assert np.array_equal(words(out, "ranges", (-1, 2)), env.cpu.find_batch(*env.flat(0))), "find() against the oracle"
    return check


@row("find_device")
def _(env, name):
    ins, n, total = reads_input()
    return Case(name, ENQUEUE, ins, {"ranges": 16 * n}, lambda p, s: env.gpu.find_device(p["pat"], p["off"], n, p["ranges"], s), oracle=find_oracle(env))


def find_variant(variant):
    def build(env, name):
        ins, n, total = reads_input()
        return Case(name, ENQUEUE, ins, {"ranges": 16 * n}, lambda p, s: env.gpu.find_device_variant(variant, p["pat"], p["off"], n, p["ranges"], s),
                    oracle=find_oracle(env))
    return build


BUILDERS["find_device_variant-2"] = find_variant(2)
BUILDERS["find_device_variant-4"] = find_variant(4)


@row("find_packed_device")
def _(env, name):
    m = 40                                                # two code words per pattern
    pair = [np.array([list(r[:m]) for r in reads[:100]], dtype=np.uint8) for reads in read_batches()]
    codes = [pack_kmers(a) for a in pair]
    n = codes[0].shape[0]

    def check(out, result):
        data, off = concat_patterns([bytes(r) for r in pair[0]])
        assert np.array_equal(words(out, "ranges", (-1, 2)), env.cpu.find_batch(data, off)), "find() of the packed patterns against the oracle"

    return Case(name, ENQUEUE, {"codes": (codes[0], codes[1])}, {"ranges": 16 * n},
                lambda p, s: env.gpu.find_packed_device(p["codes"], m, n, p["ranges"], s), oracle=check)


@row("find_stats_device")
def _(env, name):
    ins, n, total = reads_input()
    ins["stats"] = (np.zeros(8, dtype=np.uint64), u64([1000, 2000, 3000, 4000, 5000, 6000, 7000, 0]))     # stats[7] is an input: no bitmap
    return Case(name, ENQUEUE, ins, {"ranges": 16 * n}, lambda p, s: env.gpu.find_stats_device(p["pat"], p["off"], n, p["ranges"], p["stats"], s),
                inout=("stats",), oracle=find_oracle(env))


@row("lf_device")
def _(env, name):
    real, decoy = env.found_ranges()
    n = real.shape[0]
    comps = (np.arange(n, dtype=np.uint8) % 4 + 1, (np.arange(n, dtype=np.uint8) + 1) % 4 + 1)

    def check(out, result):
        assert np.array_equal(words(out, "out", (-1, 2)), env.cpu.lf_batch(real, comps[0])), "LF against the oracle"

    return Case(name, ENQUEUE, {"ranges": (real, decoy), "comps": comps}, {"out": 16 * n},
                lambda p, s: env.gpu.lf_device(p["ranges"], p["comps"], n, p["out"], s), oracle=check)


@row("count_device")
def _(env, name):
    real, decoy = env.found_ranges()
    n = real.shape[0]

    def check(out, result):
        assert np.array_equal(words(out, "counts"), env.cpu.count_batch(real)), "count() against the oracle"

    return Case(name, ENQUEUE, {"ranges": (real, decoy)}, {"counts": 8 * n}, lambda p, s: env.gpu.count_device(p["ranges"], n, p["counts"], s), oracle=check)


@row("parent_device")
def _(env, name):
    real, decoy = env.found_ranges()
    n = real.shape[0]

    def check(out, result):
        want = env.cpu.parent_batch(real)
        assert np.array_equal(words(out, "nodes"), np.ascontiguousarray(want).view(np.uint64).reshape(-1)), "parent() against the oracle"

    return Case(name, ENQUEUE, {"ranges": (real, decoy)}, {"nodes": 40 * n}, lambda p, s: env.gpu.parent_device(p["ranges"], n, p["nodes"], s), oracle=check)


@row("extend_device")
def _(env, name):
    pats, states, want = batch(BIG)
    turned = bytes.maketrans(b"ACGT", b"CGTA")
    decoy_pats = [p.translate(turned) for p in pats]
    decoy_states = u64(states).copy()
    decoy_states[:, 3], decoy_states[:, 4] = 0, env.cpu.n - 1          # other valid start ranges, the same cursors
    ins, n_patterns, total = reads_input((pats, decoy_pats))
    ins["states"] = (u64(states), decoy_states)
    n = states.shape[0]

    def check(out, result):
        assert np.array_equal(words(out, "out", (-1, 5)), want), "extend against the restatement of the walk"

    return Case(name, ENQUEUE, ins, {"out": 40 * n}, lambda p, s: env.gpu.extend_device(p["pat"], p["off"], n_patterns, p["states"], n, p["out"], s), oracle=check)


@row("kmer_windows_device")
def _(env, name):
    """The sizing call and the filling call, both on the caller's stream."""
    ins, n, total = reads_input()
    k, stride = 16, 1
    windows = sum(window_count(len(r), k, stride) for r in read_batches()[0])

    def call(p, s):
        sized_ = env.gpu.kmer_windows_device(p["pat"], p["off"], n, k, stride, 1, p["woff"], 0, 0, 0, 0, s)
        filled = env.gpu.kmer_windows_device(p["pat"], p["off"], n, k, stride, 1, 0, p["prof"], p["ranges"], p["counts"], windows, s)
        return sized_, filled

    # the window offsets are a function of the read offsets alone, which a decoy shares by rule: they cannot differ
    return Case(name, COMPLETE, ins, {"woff": 8 * (n + 1), "prof": 32 * n, "ranges": 16 * windows, "counts": 8 * windows}, call, same_by_rule=("woff",))


def cut_csr(n, first, rec_bytes):
    """The view of a seeds-and-hits call: (offsets per read, records, hit offsets, hits[, profiles]) up to the totals returned."""
    def view(raw, result):
        m, h = result
        out = {"soff": raw["soff"], "seeds": raw["seeds"][:rec_bytes * m], "hoff": raw["hoff"][:8 * (m + 1)], "hits": raw["hits"][:8 * h]}
        if "prof" in raw:
            out["prof"] = raw["prof"]
        return out
    return view


def csr_outputs(n, mcap, hcap, prof):
    out = {"soff": 8 * (n + 1), "seeds": 40 * mcap, "hoff": 8 * (mcap + 1), "hits": 8 * hcap}
    if prof:
        out["prof"] = 32 * n
    return out


@row("kmer_hits_device")
def _(env, name):
    ins, n, total = reads_input()
    k, stride = 8, 1
    host = [env.gpu.kmer_hits_batch(*env.flat(w), k, stride, HIT_MAX, True) for w in (0, 1)]
    mcap, hcap = sized(*(h[1].shape[0] for h in host)), sized(*(h[3].shape[0] for h in host))

    def check(out, result):
        from test_kmer_hits import oracle_of
        want = dict(zip(("soff", "seeds", "hoff", "hits", "prof"), oracle_of(BIG).want(k, stride, HIT_MAX, True)))
        assert result == (want["seeds"].shape[0], want["hits"].shape[0])
        for key, w in want.items():
            assert np.array_equal(words(out, key), u64(w).reshape(-1)), ("k-mer hits against the oracle", key)

    return Case(name, COMPLETE, ins, csr_outputs(n, mcap, hcap, True),
                lambda p, s: env.gpu.kmer_hits_device(p["pat"], p["off"], n, k, stride, HIT_MAX, SAMPLE, p["prof"], p["soff"], p["seeds"], mcap, p["hoff"],
                                                      p["hits"], hcap, s), view=cut_csr(n, "soff", 40), oracle=check)


@row("minimizers_device")
def _(env, name):
    ins, n, total = reads_input()
    k, w = 8, 5
    host = [env.gpu.minimizers_batch(*env.flat(x), k, w, 7) for x in (0, 1)]
    cap = sized(*(h[1].shape[0] for h in host))
    return Case(name, COMPLETE, ins, {"moff": 8 * (n + 1), "mins": 16 * cap},
                lambda p, s: env.gpu.minimizers_device(p["pat"], p["off"], n, k, w, 7, p["moff"], p["mins"], cap, s),
                view=lambda raw, total_: {"moff": raw["moff"], "mins": raw["mins"][:16 * total_]})


@row("minimizer_hits_device")
def _(env, name):
    ins, n, total = reads_input()
    k, w = 16, 5
    host = [env.gpu.minimizer_hits_batch(*env.flat(x), k, w, 7, HIT_MAX, True) for x in (0, 1)]
    mcap, hcap = sized(*(h[1].shape[0] for h in host)), sized(*(h[3].shape[0] for h in host))
    return Case(name, COMPLETE, ins, csr_outputs(n, mcap, hcap, True),
                lambda p, s: env.gpu.minimizer_hits_device(p["pat"], p["off"], n, k, w, 7, HIT_MAX, SAMPLE, p["prof"], p["soff"], p["seeds"], mcap, p["hoff"],
                                                           p["hits"], hcap, s), view=cut_csr(n, "soff", 40))


@row("capped_seeds_device")
def _(env, name):
    ins, n, total = reads_input()
    args = (8, 0, 4)                                      # min_length, max_length, max_count
    host = [env.gpu.capped_seeds_batch(*env.flat(x), *args, HIT_MAX, True) for x in (0, 1)]
    mcap, hcap = sized(*(h[1].shape[0] for h in host)), sized(*(h[3].shape[0] for h in host))
    return Case(name, COMPLETE, ins, csr_outputs(n, mcap, hcap, False),
                lambda p, s: env.gpu.capped_seeds_device(p["pat"], p["off"], n, *args, HIT_MAX, SAMPLE, p["soff"], p["seeds"], mcap, p["hoff"], p["hits"], hcap, s),
                view=cut_csr(n, "soff", 40))


def support_buffers(n_bins):
    """The support array is added into: what it held when the kernels ran shows in the result."""
    return (np.arange(n_bins, dtype=np.uint64) * np.uint64(3), np.arange(n_bins, dtype=np.uint64)[::-1] * np.uint64(5) + np.uint64(1 << 40))


def frozen(stats):
    return None if stats is None else tuple(sorted(stats.items()))


@row("kmer_support_device")
def _(env, name):
    ins, n, total = reads_input()
    n_bins = env.n_bins()
    ins["support"] = support_buffers(n_bins)
    return Case(name, COMPLETE, ins, {}, lambda p, s: frozen(env.gpu.kmer_support_device(p["pat"], p["off"], n, 16, 1, HIT_MAX, SHIFT, 0, p["support"], n_bins, s)),
                inout=("support",))


@row("seed_support_device")
def _(env, name):
    real, decoy = env.seeds()
    m, n_bins = real.shape[0], env.n_bins()
    ins = {"seeds": (real, decoy), "weights": (np.arange(m, dtype=np.uint64) % np.uint64(5), np.arange(m, dtype=np.uint64) % np.uint64(3) + np.uint64(1)),
           "support": support_buffers(n_bins)}
    return Case(name, COMPLETE, ins, {}, lambda p, s: frozen(env.gpu.seed_support_device(p["seeds"], m, p["weights"], 0, SHIFT, 0, p["support"], n_bins, s)),
                inout=("support",))


@row("index_kmer_support_device")
def _(env, name):
    n_bins = env.n_bins()
    return Case(name, COMPLETE, {"support": support_buffers(n_bins)}, {},
                lambda p, s: frozen(env.gpu.index_kmer_support_device(8, HIT_MAX, SHIFT, 0, p["support"], n_bins, stream=s)), inout=("support",))


def class_table(env, n_classes):
    t = (np.arange(env.n_bins(), dtype=np.uint64) * np.uint64(2654435761) % np.uint64(n_classes)).astype(np.uint32)
    return (t, t)


def seed_groups(m, per=7):
    g = u64(np.arange(0, m + 1, per))
    return g, g.shape[0] - 1


@row("kmer_classes_device")
def _(env, name):
    ins, n, total = reads_input()
    n_classes = 5
    ins["table"] = class_table(env, n_classes)
    return Case(name, COMPLETE, ins, {"votes": 8 * n * n_classes, "calls": 48 * n},
                lambda p, s: frozen(env.gpu.kmer_classes_device(p["pat"], p["off"], n, 8, 1, HIT_MAX, SHIFT, 0, p["table"], env.n_bins(), n_classes, p["votes"],
                                                                p["calls"], s)))


@row("seed_classes_device")
def _(env, name):
    real, decoy = env.seeds()
    m, n_classes = real.shape[0], 5
    goff, n_groups = seed_groups(m)
    ins = {"goff": (goff, goff), "seeds": (real, decoy), "table": class_table(env, n_classes)}
    return Case(name, COMPLETE, ins, {"votes": 8 * n_groups * n_classes, "calls": 48 * n_groups},
                lambda p, s: frozen(env.gpu.seed_classes_device(p["goff"], n_groups, p["seeds"], m, 0, 0, SHIFT, 0, p["table"], env.n_bins(), n_classes,
                                                                p["votes"], p["calls"], s)))


@row("kmer_top_classes_device")
def _(env, name):
    ins, n, total = reads_input()
    n_classes, top_n = 5000, 3                            # beyond the 4096 classes of the dense form
    ins["table"] = class_table(env, n_classes)
    return Case(name, COMPLETE, ins, {"top": 16 * n * top_n, "sums": 24 * n},
                lambda p, s: frozen(env.gpu.kmer_top_classes_device(p["pat"], p["off"], n, 16, 1, HIT_MAX, SHIFT, 0, p["table"], env.n_bins(), n_classes, top_n,
                                                                    p["top"], p["sums"], s)))


@row("seed_top_classes_device")
def _(env, name):
    real, decoy = env.seeds()
    m, n_classes, top_n = real.shape[0], 5000, 3
    goff, n_groups = seed_groups(m)
    ins = {"goff": (goff, goff), "seeds": (real, decoy), "table": class_table(env, n_classes)}
    return Case(name, COMPLETE, ins, {"top": 16 * n_groups * top_n, "sums": 24 * n_groups},
                lambda p, s: frozen(env.gpu.seed_top_classes_device(p["goff"], n_groups, p["seeds"], m, 0, 0, SHIFT, 0, p["table"], env.n_bins(), n_classes, top_n,
                                                                    p["top"], p["sums"], s)))


def seed_clusters(sizes, knob):
    """One group per tier.  The decoy keeps every offset and moves the hits and the seeds' positions."""
    def build(env, name):
        goff, seeds, hoff, hits = synthetic(np.random.default_rng(0x57E4), sizes)
        other = np.random.default_rng(0x57E5)
        d_seeds = seeds.copy()
        d_seeds[:, 0] = u64(other.integers(0, 200, seeds.shape[0]))
        d_hits = u64(other.integers(1000, (1 << 16) - 1000, hits.shape[0]))
        cmap = identity_map(1 << 16)
        n_groups, top_n, band = goff.shape[0] - 1, 5, 7
        ins = {"goff": (goff, goff), "seeds": (seeds, d_seeds), "hoff": (hoff, hoff), "hits": (hits, d_hits), "cmap": (cmap, cmap)}

        def call(p, s):
            before = os.environ.get("GCSA2_CLUSTER_LDS")
            if knob is not None:
                os.environ["GCSA2_CLUSTER_LDS"] = knob
            try:
                stats = env.gpu.seed_clusters_device(p["goff"], n_groups, p["seeds"], seeds.shape[0], p["hoff"], p["hits"], hits.shape[0], 0, p["cmap"],
                                                     cmap.shape[0], band, top_n, p["top"], p["sums"], s)
            finally:
                if knob is not None:
                    if before is None:
                        del os.environ["GCSA2_CLUSTER_LDS"]
                    else:
                        os.environ["GCSA2_CLUSTER_LDS"] = before
            assert (stats["spilled"] > 0) == (knob is not None), stats
            return frozen(stats)

        return Case(name, COMPLETE, ins, {"top": 64 * n_groups * top_n, "sums": 24 * n_groups}, call)
    return build


BUILDERS["seed_clusters_device"] = seed_clusters([200, 3000, 0, 30], None)            # at most 256 anchors, at most 4096
BUILDERS["seed_clusters_device-lds64"] = seed_clusters([200, 40, 70], "64")           # above GCSA2_CLUSTER_LDS=64: the spill path


def coord_table(env):
    t = np.arange(env.n_bins(), dtype=np.uint64) << np.uint64(SHIFT)
    return (t, t)


@row("kmer_clusters_device")
def _(env, name):
    ins, n, total = reads_input()
    top_n = 2
    ins["cmap"] = coord_table(env)
    return Case(name, COMPLETE, ins, {"top": 64 * n * top_n, "sums": 24 * n},
                lambda p, s: frozen(env.gpu.kmer_clusters_device(p["pat"], p["off"], n, 8, 1, HIT_MAX, SAMPLE, SHIFT, p["cmap"], env.n_bins(), 7, top_n, p["top"],
                                                                 p["sums"], s)))


@row("minimizer_clusters_device")
def _(env, name):
    ins, n, total = reads_input()
    top_n = 2
    ins["cmap"] = coord_table(env)
    return Case(name, COMPLETE, ins, {"top": 64 * n * top_n, "sums": 24 * n},
                lambda p, s: frozen(env.gpu.minimizer_clusters_device(p["pat"], p["off"], n, 16, 5, 7, HIT_MAX, SAMPLE, SHIFT, p["cmap"], env.n_bins(), 7, top_n,
                                                                      p["top"], p["sums"], s)))


def match_stats(variant, sized_):
    def build(env, name):
        ins, n, total = reads_input()

        def check(out, result):
            ms, rng, fb = env.cpu.match_stats_batch(*env.flat(0))
            assert np.array_equal(out["ms"].view(np.uint16), ms) and np.array_equal(words(out, "ranges", (-1, 2)), rng), "match_stats against the oracle"
            assert np.array_equal(words(out, "fb"), fb), "parent() calls against the oracle"

        return Case(name, ENQUEUE if sized_ else ONE_WAIT, ins, {"ms": 2 * (total + 4), "ranges": 16 * n, "fb": 8 * n},
                    lambda p, s: env.gpu.match_stats_device(p["pat"], p["off"], n, p["ms"], p["ranges"], p["fb"], s, variant, total if sized_ else None),
                    view=lambda raw, result: {"ms": raw["ms"][:2 * total], "ranges": raw["ranges"], "fb": raw["fb"]}, oracle=check)
    return build


BUILDERS["match_stats_device-0"] = match_stats(0, False)
BUILDERS["match_stats_device-2"] = match_stats(2, False)
BUILDERS["match_stats_device-5-sized"] = match_stats(5, True)


@row("match_stats_profile_device")
def _(env, name):
    ins, n, total = reads_input()
    ins["prof"] = (np.zeros(16, dtype=np.uint64), np.zeros(16, dtype=np.uint64))          # zeroed by the caller; cycle counts: not compared
    return Case(name, ENQUEUE, ins, {"ms": 2 * (total + 4), "ranges": 16 * n, "fb": 8 * n},
                lambda p, s: env.gpu.match_stats_profile_device(p["pat"], p["off"], n, total, p["ms"], p["ranges"], p["fb"], p["prof"], s),
                view=lambda raw, result: {"ms": raw["ms"][:2 * total], "ranges": raw["ranges"], "fb": raw["fb"]})


def match_breaks(max_length):
    def build(env, name):
        ins, n, total = reads_input()
        host = [env.gpu.match_breaks_batch(*env.flat(x), 0, max_length=max_length) for x in (0, 1)]
        cap = sized(*(h[1].shape[0] for h in host))
        return Case(name, COMPLETE, ins, {"boff": 8 * (n + 1), "breaks": 32 * cap, "ranges": 16 * n, "fb": 8 * n},
                    lambda p, s: env.gpu.match_breaks_device(p["pat"], p["off"], n, total, p["boff"], p["breaks"], cap, p["ranges"], p["fb"], s, 0, 0, max_length),
                    view=lambda raw, t: {"boff": raw["boff"], "breaks": raw["breaks"][:32 * t], "ranges": raw["ranges"], "fb": raw["fb"]})
    return build


BUILDERS["match_breaks_device"] = match_breaks(0)
BUILDERS["match_breaks_device-bounded"] = match_breaks(12)


def mem_hits(max_length):
    def build(env, name):
        ins, n, total = reads_input()
        host = [env.gpu.mem_hits_batch(*env.flat(x), 8, HIT_MAX, True, max_length=max_length) for x in (0, 1)]
        mcap, hcap = sized(*(h[1].shape[0] for h in host)), sized(*(h[3].shape[0] for h in host))
        return Case(name, COMPLETE, ins, csr_outputs(n, mcap, hcap, False),
                    lambda p, s: env.gpu.mem_hits_device(p["pat"], p["off"], n, total, 8, HIT_MAX, SAMPLE, p["soff"], p["seeds"], mcap, p["hoff"], p["hits"], hcap,
                                                         s, max_length), view=cut_csr(n, "soff", 40))
    return build


BUILDERS["mem_hits_device"] = mem_hits(0)
BUILDERS["mem_hits_device-bounded"] = mem_hits(12)


@row("sub_mem_hits_device")
def _(env, name):
    """The reads and the MEM offsets are shared; the decoy's records are other valid matches of the same reads: every MEM of
    two or more characters without its first character, with find() and count() of what is left."""
    reads = read_batches()[0]
    data, off = env.flat(0)
    total, n = int(off[-1]), len(reads)
    moff, mems, _, _ = env.gpu.mem_hits_batch(data, off, 8, HIT_MAX, True)
    mems = u64(mems)
    decoy = mems.copy()
    read_of = np.repeat(np.arange(n), np.diff(moff.astype(np.int64)))
    for i in range(mems.shape[0]):
        pos, length = int(mems[i, 0]), int(mems[i, 1])
        if length >= 2:
            sp, ep = env.cpu.find(reads[read_of[i]][pos + 1:pos + length])
            decoy[i] = (pos + 1, length - 1, sp, ep, env.cpu.count((sp, ep)))
    nm = mems.shape[0]
    args = (4, 8)                                         # min_length, reseed_length
    host = [env.gpu.sub_mem_hits_batch(data, off, moff, x, *args, HIT_MAX, True) for x in (mems, decoy)]
    scap, hcap = sized(*(h[1].shape[0] for h in host)), sized(*(h[3].shape[0] for h in host))
    assert host[0][1].shape[0] > 0
    ins = {"pat": (data[:total], data[:total]), "off": (off, off), "moff": (u64(moff), u64(moff)), "mems": (mems, decoy)}
    return Case(name, COMPLETE, ins, csr_outputs(nm, scap, hcap, False),
                lambda p, s: env.gpu.sub_mem_hits_device(p["pat"], p["off"], n, total, p["moff"], p["mems"], nm, *args, HIT_MAX, SAMPLE, p["soff"], p["seeds"],
                                                         scap, p["hoff"], p["hits"], hcap, s), view=cut_csr(nm, "soff", 40))


# ---- locate: one range per size class of removeDuplicates --------------------------------------------------------------------

SEGMENT_WIDTHS = (1, 9, 300, 3000, 9000)                  # 1, 2..16, 17..1024, 1025..8192, more than 8192; and the whole index


def segment_ranges(n):
    real = [(11 + 13 * w, 11 + 13 * w + w - 1) for w in SEGMENT_WIDTHS] + [(0, n - 1), (5, 4)]
    decoy = [(401 + 7 * w, 401 + 7 * w + w - 1) for w in SEGMENT_WIDTHS] + [(1, n - 2), (9, 8)]
    assert all(b < n for _, b in real + decoy)
    return u64(real), u64(decoy)


def locate_into(sort):
    def build(env, name):
        real, decoy = segment_ranges(env.seg_n)
        nq = real.shape[0]
        want = [env.seg_cpu.locate_batch(r, threads=8) for r in (real, decoy)]
        raw_total = [sum(len(env.seg_cpu.locate((int(a), int(b)), sort=False)) for a, b in r) for r in (real, decoy)]
        cap = sized(*raw_total)                            # room for the values before deduplication: sorted in place

        def check(out, result):
            if sort:
                assert np.array_equal(words(out, "off"), want[0][0]) and np.array_equal(words(out, "values"), want[0][1]), "locate() against the oracle"
            else:
                flat = np.concatenate([np.asarray(env.seg_cpu.locate((int(a), int(b)), sort=False), dtype=np.uint64) for a, b in real])
                assert np.array_equal(words(out, "values"), flat), "locate(sort = false) against the oracle"

        return Case(name, COMPLETE, {"ranges": (real, decoy)}, {"off": 8 * (nq + 1), "values": 8 * cap},
                    lambda p, s: env.seg_gpu.locate_into(p["ranges"], nq, p["off"], p["values"], cap, s, bool(sort)),
                    view=lambda raw, total: {"off": raw["off"], "values": raw["values"][:8 * total]}, oracle=check)
    return build


BUILDERS["locate_into-sorted"] = locate_into(True)
BUILDERS["locate_into-unsorted"] = locate_into(False)


@functools.lru_cache(maxsize=None)
def hip_runtime():
    import torch  # noqa: F401  (maps the runtime the library uses)
    for soname in ("libamdhip64.so.7", "libamdhip64.so"):
        try:
            return ctypes.CDLL(soname)
        except OSError:
            continue
    raise AssertionError("the HIP runtime is not loadable")


@row("locate_device")
def _(env, name):
    """The job interface: the result lives in the job's own memory, and is copied out here on the caller's stream."""
    real, decoy = segment_ranges(env.seg_n)
    nq = real.shape[0]
    want = [env.seg_cpu.locate_batch(r, threads=8) for r in (real, decoy)]
    cap = sized(*(int(w[0][-1]) for w in want))
    hip = hip_runtime()
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    hip.hipStreamQuery.argtypes = [ctypes.c_void_p]
    hip.hipStreamSynchronize.argtypes = [ctypes.c_void_p]

    def call(p, s):
        job, d_off, d_val, total = env.seg_gpu.locate_device(p["ranges"], nq, s, True)
        try:
            assert hip.hipStreamQuery(s) == 0, "work left on the stream of a call that is complete on return"
            assert total <= cap
            assert hip.hipMemcpyAsync(p["off"], d_off, 8 * (nq + 1), 3, s) == 0
            assert total == 0 or hip.hipMemcpyAsync(p["values"], d_val, 8 * total, 3, s) == 0
            assert hip.hipStreamSynchronize(s) == 0
        finally:
            env.seg_gpu.locate_discard(job)
        return total

    def check(out, result):
        assert np.array_equal(words(out, "off"), want[0][0]) and np.array_equal(words(out, "values"), want[0][1]), "locate() against the oracle"

    return Case(name, COMPLETE, {"ranges": (real, decoy)}, {"off": 8 * (nq + 1), "values": 8 * cap}, call,
                view=lambda raw, total: {"off": raw["off"], "values": raw["values"][:8 * total]}, oracle=check)


LMAX = 1100                                               # beyond the 1024 values one wavefront keeps in LDS


@row("locate_max_into")
def _(env, name):
    """One range beyond the LDS budget of the kernel (min(max_positions, count) > 1024: the per-range path), the same one with
    max_positions below its count, and small ones that stay in the kernel."""
    from test_locate_max_batch import reference_spins
    n = env.seg_n
    real = [(0, n - 1), (20, 20), (700, 730), (5, 4), (4000, 4007)]
    decoy = [(1, n - 2), (21, 21), (900, 930), (9, 8), (5000, 5007)]
    for r in real + decoy:
        assert not reference_spins(env.seg_cpu, r, LMAX), r
    assert env.seg_cpu.count(real[0]) > LMAX > 1024
    real, decoy = u64(real), u64(decoy)
    nq = real.shape[0]
    # the values need room for the slots, min(max_positions, count()) per range, which are closed up afterwards
    cap = sized(*(sum(min(LMAX, env.seg_cpu.count((int(a), int(b)))) for a, b in r) for r in (real, decoy)))

    def check(out, result):
        want = np.concatenate([np.asarray(env.seg_cpu.locate((int(a), int(b)), max_positions=LMAX), dtype=np.uint64) for a, b in real])
        assert np.array_equal(words(out, "values"), want), "locate(range, max_positions) against the oracle"

    return Case(name, COMPLETE, {"ranges": (real, decoy)}, {"off": 8 * (nq + 1), "values": 8 * cap},
                lambda p, s: env.seg_gpu.locate_max_into(p["ranges"], nq, LMAX, p["off"], p["values"], cap, s),
                view=lambda raw, total: {"off": raw["off"], "values": raw["values"][:8 * total]}, oracle=check)


# ---- range packing -------------------------------------------------------------------------------------------------------------

def pack_case(bits):
    def build(env, name):
        real, decoy = env.all_ranges()
        n = real.shape[0]
        if bits == 48:
            real, decoy = real.copy(), decoy.copy()
            real[3], real[n // 2], decoy[5] = (0, env.cpu.n - 1), (7, 400), (2, 900)       # ranges of 255 and more path nodes: the overflow list
            capacity = 8
            size = env.engine.wire48_bytes(n, capacity)

            def view(raw, result):
                body = (6 * n + 15) & ~15
                count = int(raw["packed"][body:body + 8].view(np.uint64)[0])
                assert count <= capacity
                listed = raw["packed"][body + 16:body + 16 + 16 * min(count, capacity)].view(np.uint64).reshape(-1, 2)
                return {"ranges": raw["packed"][:6 * n], "count": u64([count]), "list": listed[np.argsort(listed[:, 0])]}     # appended in any order

            # (the library clears the list's count itself, on the caller's stream: the block starts sentinel-filled like any output)
            return Case(name, ENQUEUE, {"ranges": (real, decoy)}, {"packed": size},
                        lambda p, s: env.engine.pack_ranges48_device(p["ranges"], n, p["packed"], capacity, s), view=view)
        call = {32: env.engine.pack_ranges32_device, 40: env.engine.pack_ranges40_device}[bits]
        return Case(name, ENQUEUE, {"ranges": (real, decoy)}, {"packed": {32: 8, 40: 10}[bits] * n}, lambda p, s: call(p["ranges"], n, p["packed"], s))
    return build


def unpack_case(bits):
    def build(env, name):
        import torch
        pair = env.all_ranges()
        n = pair[0].shape[0]
        capacity = 8
        packed = []
        for which in (0, 1):                              # the library's own packing of either batch, made on the default stream
            rng = pair[which].copy()
            if bits == 48:                                # ranges of 255 and more path nodes: one in the real batch, two in the decoy
                rng[3 + which] = (which, 700 + which)
                if which:
                    rng[10] = (5, 900)
            d_rng = torch.from_numpy(rng.view(np.int64).copy()).to("cuda:0")
            size = {32: 8 * n, 40: 10 * n, 48: env.engine.wire48_bytes(n, capacity)}[bits]
            d_packed = torch.zeros(size + 16, dtype=torch.uint8, device="cuda:0")
            if bits == 48:
                env.engine.pack_ranges48_device(d_rng.data_ptr(), n, d_packed.data_ptr(), capacity, 0)
            else:
                {32: env.engine.pack_ranges32_device, 40: env.engine.pack_ranges40_device}[bits](d_rng.data_ptr(), n, d_packed.data_ptr(), 0)
            torch.cuda.synchronize()
            packed.append((d_packed[:size].cpu().numpy(), rng))

        def check(out, result):
            assert np.array_equal(words(out, "ranges", (-1, 2)), packed[0][1]), "unpack(pack(ranges)) == ranges"

        if bits == 48:
            call = lambda p, s: env.engine.unpack_ranges48_device(p["packed"], n, capacity, p["ranges"], p["long"], s)     # noqa: E731
            return Case(name, ENQUEUE, {"packed": (packed[0][0], packed[1][0])}, {"ranges": 16 * n, "long": 8}, call, oracle=check)
        call = {32: env.engine.unpack_ranges32_device, 40: env.engine.unpack_ranges40_device}[bits]
        return Case(name, ENQUEUE, {"packed": (packed[0][0], packed[1][0])}, {"ranges": 16 * n}, lambda p, s: call(p["packed"], n, p["ranges"], s), oracle=check)
    return build


for _bits in (32, 40, 48):
    BUILDERS[f"pack_ranges{_bits}_device"] = pack_case(_bits)
    BUILDERS[f"unpack_ranges{_bits}_device"] = unpack_case(_bits)


# ---- GPU -------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def engine():
    from gcsa2_amd import binding
    assert binding.device_count() >= 1, "no MI355X visible"
    return binding


@pytest.fixture(scope="module")
def env(engine):
    from oracle.oracle import OracleIndex
    from workload import builder, graphs
    gpu, _ = engine.open_index(indexed(BIG)[0], device=0)
    g = graphs.snp_graph(30000, 0x4D1, 0x4D2, snp_period=5, node_len=16)          # the index of test_locate_segment_sizes
    ix = builder.build(g, 16, sample_period=16)
    seg_gpu, _ = engine.open_index(ix, device=0)
    e = Env(engine, gpu, seg_gpu, OracleIndex(ix), ix.n)
    e.cases = {}
    yield e
    import torch
    torch.cuda.synchronize()
    seg_gpu.close()
    gpu.close()


def case_of(env, name):
    if name not in env.cases:
        case = BUILDERS[name](env, name)
        assert case.contract == TABLE[name][1], name
        env.cases[name] = case
    return env.cases[name]


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(TABLE))
def test_entry_point_on_a_caller_stream(env, name):
    """Both probes (and, where the header promises it, nothing left on the stream when the call returns) for one row."""
    case = case_of(env, name)
    print(f"stream_contract timing: {name} {case.time_ms():.3f} ms (delay {streams.DELAY_MS:.0f} ms)")
    streams.probe_delayed_inputs(case)
    streams.probe_busy_null_stream(case)


@pytest.mark.gpu
def test_the_probe_sees_a_wrong_stream(env):
    """The control: with S delayed as in the first probe, find_device and count_device are issued on a SECOND stream and only
    that one is waited for.  They must give the decoy's results: torch's streams do not order against each other, and the delay
    outlasts a call.  (No change to the library is needed for this: the caller is the one who picks the wrong stream.)"""
    import torch
    for name in ("find_device", "count_device"):
        case = case_of(env, name)
        want_real, want_decoy = case.expected(0), case.expected(1)
        case.assert_not_vacuous()
        ins, outs = case.device_inputs(1), case.device_outputs()
        real = case.pinned(0)
        S = torch.cuda.Stream()
        ready = torch.cuda.Event()
        torch.cuda.synchronize()
        try:
            with torch.cuda.stream(S):
                streams.delay(3 * streams.DELAY_MS)          # (room for the search for a stream that runs beside S)
                for key, t in ins.items():
                    t[:real[key].shape[0]].copy_(real[key], non_blocking=True)
                ready.record(S)
            other = streams.independent_stream(ready)
            assert not ready.query(), (name, "the delay had ended before the call was issued: inconclusive")
            result = case.run(ins, outs, other.cuda_stream)
            other.synchronize()
            assert not ready.query(), (name, "the delay did not outlast the call")
            got = case.collect(ins, outs, result, "control", stream=other)
            case.assert_equal(got, want_decoy, "the wrong stream sees the decoy")
            assert any(not np.array_equal(got[0][key], want_real[0][key]) for key in got[0]), name
        finally:
            torch.cuda.synchronize()


ENQUEUE_ROTATION = ("find_device", "lf_device", "count_device", "parent_device", "extend_device", "pack_ranges32_device", "unpack_ranges32_device",
                    "pack_ranges40_device", "unpack_ranges40_device", "pack_ranges48_device", "unpack_ranges48_device")


@pytest.mark.gpu
def test_two_streams_interleaved(env):
    """One thread, two streams: the enqueue-only calls alternately on S1 (the real batch) and S2 (the decoy batch), three rounds
    each without a wait in between; every output of every round is exact."""
    import torch
    S = (torch.cuda.Stream(), torch.cuda.Stream())
    cases = [case_of(env, name) for name in ENQUEUE_ROTATION]
    want = {(c.name, which): c.expected(which) for c in cases for which in (0, 1)}
    ins = {(c.name, which): c.device_inputs(which) for c in cases for which in (0, 1)}
    outs = {(c.name, which, r): c.device_outputs() for c in cases for which in (0, 1) for r in range(3)}
    # a call that adds into one of its inputs gets that input afresh every round
    fresh = {(c.name, which, r): (c.device_inputs(which) if c.inout else ins[(c.name, which)]) for c in cases for which in (0, 1) for r in range(3)}
    torch.cuda.synchronize()
    results = {}
    try:
        for r in range(3):
            for c in cases:
                for which in (0, 1):
                    results[(c.name, which, r)] = c.run(fresh[(c.name, which, r)], outs[(c.name, which, r)], S[which].cuda_stream)
        S[0].synchronize()
        S[1].synchronize()
        for (name, which, r), result in results.items():
            c = env.cases[name]
            c.assert_equal(c.collect(fresh[(name, which, r)], outs[(name, which, r)], result, "interleaved"), want[(name, which)], ("interleaved", which, r))
    finally:
        torch.cuda.synchronize()


CONCURRENT_ROTATION = ("kmer_hits_device", "capped_seeds_device", "mem_hits_device", "sub_mem_hits_device", "kmer_classes_device", "kmer_clusters_device",
                       "locate_into-sorted", "locate_max_into", "match_stats_device-0")
THREADS, ROUNDS = 6, 4


@pytest.mark.gpu
def test_concurrent_callers_on_streams(env):
    """Six host threads share the handles, each on a stream of its own, four rounds of a rotation over nine features that is
    offset per thread, so that different features overlap: arena hand-over, result slots, staging pool and memory pool under
    real overlap.  Every output is compared exactly with what the call gave alone; errors are asserted in the main thread."""
    import torch
    cases = [case_of(env, name) for name in CONCURRENT_ROTATION]
    want = {c.name: c.expected(0) for c in cases}
    plan = {}
    for t in range(THREADS):
        for r in range(ROUNDS):
            for i in range(len(cases)):
                c = cases[(i + t * 2 + r) % len(cases)]
                plan[(t, r, i)] = (c, c.device_inputs(0), c.device_outputs())
    stream_of = [torch.cuda.Stream() for _ in range(THREADS)]
    torch.cuda.synchronize()
    errors, start = [], threading.Barrier(THREADS)

    def worker(t):
        try:
            S = stream_of[t]
            start.wait()
            for r in range(ROUNDS):
                done = []
                for i in range(len(cases)):
                    c, ins, outs = plan[(t, r, i)]
                    done.append((c, ins, outs, c.run(ins, outs, S.cuda_stream)))
                S.synchronize()
                for c, ins, outs, result in done:
                    c.assert_equal(c.collect(ins, outs, result, "concurrent", stream=S), want[c.name], ("thread", t, "round", r))
        except Exception as e:          # noqa: BLE001  (reported below, in the main thread)
            errors.append((t, repr(e)))
            start.abort()

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(THREADS)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    torch.cuda.synchronize()
    assert not errors, errors[:3]
