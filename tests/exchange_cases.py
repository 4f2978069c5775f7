"""Case tables and plain numpy references of the gradient-exchange kernels (csrc/hm_exchange.hip), shared by
test_exchange_cases_cpu.py (which checks this file) and test_exchange_gpu.py (which checks the kernels against it).

No GPU code and no torch here: the references work on raw int32 / float32 / uint32 numpy arrays, slot by slot or with
numpy's elementwise float32 arithmetic, which rounds every operation once and never contracts a multiply and an add.
Every comparison built on them is bit-exact, so float data is compared through its int32 view (NaN payloads, -0.0).

Layout of a list buffer, as parallel.StaticGradExchange builds it: [n_lists, stride] int32; a table with capacity cap
and F features owns the words [offset, offset + cap * (1 + F)) of every list, entry = [row | F values as fp32 bits]."""
import numpy as np

I32, U32, F32, F64 = np.int32, np.uint32, np.float32, np.float64
U = 2.0 ** -24                      # unit roundoff of fp32

# ---- hm_rows_pack ----------------------------------------------------------------------------------------------------
TOTAL_ROWS = 4099                   # 128 full bits words and one with 3 valid bits
PACK_F = (1, 2, 3, 8)
PACK_CAP = 300                      # two blocks of 256 threads, the second partial
PACK_COUNTS = (0, 1, 255, 256, 257, PACK_CAP)
PACK_OVER = 37                      # the overflow case claims cap + 37 rows
SPECIAL_BITS = (0x80000000, 0x7f800000, 0x7fc01234, 0x00000001)      # -0.0, +inf, a quiet NaN with payload, a subnormal
GUARD = 0x5a5a5a5a                  # guard / sentinel word (as a float: 1.5e16; as a row: far out of range)


def _as_i32(words):
    return np.asarray(words, dtype=np.int64).astype(U32).view(I32)


def pack_inputs(F, seed=0):
    """dense [TOTAL_ROWS, F] fp32 (nonzero everywhere, the special values in the first listed rows), rows [cap + 37]
    int32 (unique; rows[0] = 0, rows[1] = TOTAL_ROWS - 1), bits [ceil(TOTAL_ROWS / 32)] uint32 with the bit of every
    listed row AND of `extra` rows that are claimed but not listed; 40 words hold three listed and two extra bits"""
    rs = np.random.RandomState(1000 * F + seed)
    n_list = PACK_CAP + PACK_OVER
    shared, extra = [], [1, 31, TOTAL_ROWS - 2]              # neighbours of row 0 and of the last row (partial word)
    for w in rs.choice(np.arange(1, TOTAL_ROWS // 32), 40, replace=False):
        b = rs.choice(32, 5, replace=False)
        shared += [32 * int(w) + int(k) for k in b[:3]]
        extra += [32 * int(w) + int(k) for k in b[3:]]
    taken = set(shared) | set(extra) | {0, TOTAL_ROWS - 1}
    pool = np.array([r for r in range(TOTAL_ROWS) if r not in taken])
    rest = rs.choice(pool, n_list - 2 - len(shared), replace=False)
    tail = np.concatenate([np.array(shared), rest])
    rs.shuffle(tail)
    rows = np.concatenate([[0, TOTAL_ROWS - 1], tail]).astype(I32)
    dense = rs.standard_normal((TOTAL_ROWS, F)).astype(F32)
    dense[dense == 0] = 1.0
    di = dense.view(I32)
    for k, sb in enumerate(SPECIAL_BITS * 2):                # slots 0 .. 7, feature k % F (slot 0 is in every count >= 1)
        di[rows[k], k % F] = _as_i32([sb])[0]
    di[rows[0], 0] = _as_i32([SPECIAL_BITS[2]])[0]           # the NaN payload travels in the count = 1 case too
    bits = np.zeros((TOTAL_ROWS + 31) // 32, dtype=U32)
    for r in list(rows) + extra:
        bits[r >> 5] |= U32(1) << U32(r & 31)
    return dict(dense=dense, rows=rows, bits=bits, extra=np.array(extra, dtype=I32))


def pack_ref(dense, rows, count, cap, bits, status):
    """hm_rows_pack: (payload [cap, 1 + F] int32, dense after, bits after, status after).  status None = NULL"""
    F = dense.shape[1]
    d = dense.view(I32).copy()
    b = bits.copy()
    payload = np.zeros((cap, 1 + F), dtype=I32)
    payload[:, 0] = -1
    for slot in range(min(int(count), cap)):
        r = int(rows[slot])
        payload[slot, 0] = r
        payload[slot, 1:] = d[r]
        d[r] = 0
        b[r >> 5] &= ~(U32(1) << U32(r & 31))
    if status is not None and count > cap:
        status = max(int(status), int(count) - cap)
    return payload, d.view(F32), b, status


# ---- hm_rows_apply / hm_rows_clear -----------------------------------------------------------------------------------
N_LISTS = (1, 2, 3, 8)
SCALES = (1.0, 0.5, 1.0 / 3.0, 0.125)
# two tables in one buffer: name -> (total_rows, F, cap); B starts where A ends, the stride leaves slack after B
TABLES = {"A": (TOTAL_ROWS, 2, 300), "B": (2053, 8, 261)}
OFFSETS = {"A": 0, "B": TABLES["A"][2] * (1 + TABLES["A"][1])}
SLACK = 11
STRIDE = OFFSETS["B"] + TABLES["B"][2] * (1 + TABLES["B"][1]) + SLACK
N_SHARED, N_SKIP = 60, 10           # rows every list names; entries per list of each of the four skipped kinds
SLACK_ROW = 3                       # slack words alternate (SLACK_ROW, bits of 1.0f): read as an entry, row 3 would move


def skipped_rows(total_rows):
    return (-1, -5, total_rows, total_rows + 7)


def _normal_values(rs, shape):
    """fp32 of magnitude 2^-7 .. 2^7: sums and products of a few of them stay normal"""
    v = rs.uniform(2.0 ** -7, 2.0 ** 7, shape) * rs.choice([-1.0, 1.0], shape)
    return v.astype(F32)


def list_segment(name, n_lists, seed=0):
    """[n_lists, cap, 1 + F] int32 entries of table `name`: N_SHARED rows in every list (at different slots), a disjoint
    set of rows per list, N_SKIP entries of each skipped kind (with nonzero values), shuffled; row SLACK_ROW and many
    others in no list"""
    total, F, cap = TABLES[name]
    rs = np.random.RandomState(77 + 13 * n_lists + seed + (0 if name == "A" else 5))
    own = cap - N_SHARED - 4 * N_SKIP
    perm = rs.permutation(np.setdiff1d(np.arange(total), [SLACK_ROW]))
    assert N_SHARED + n_lists * own <= perm.size
    seg = np.zeros((n_lists, cap, 1 + F), dtype=I32)
    for r in range(n_lists):
        rows = np.concatenate([perm[:N_SHARED], perm[N_SHARED + r * own:N_SHARED + (r + 1) * own],
                               np.repeat(skipped_rows(total), N_SKIP)])
        rs.shuffle(rows)
        seg[r, :, 0] = rows
        seg[r, :, 1:] = _normal_values(rs, (cap, F)).view(I32)
    return seg


def lists_buffer(n_lists, seed=0):
    """the [n_lists, STRIDE] buffer of both tables, slack words alternating (SLACK_ROW, bits of 1.0f)"""
    buf = np.empty((n_lists, STRIDE), dtype=I32)
    for name, (total, F, cap) in TABLES.items():
        o = OFFSETS[name]
        buf[:, o:o + cap * (1 + F)] = list_segment(name, n_lists, seed).reshape(n_lists, -1)
    slack = np.array([SLACK_ROW, F32(1.0).view(I32)] * SLACK, dtype=I32)[:SLACK]
    buf[:, STRIDE - SLACK:] = slack
    return buf


def accumulator(name, seed=0):
    """a dense table that is nonzero (and normal) everywhere"""
    total, F, _ = TABLES[name]
    return _normal_values(np.random.RandomState(501 + seed + (0 if name == "A" else 1)), (total, F))


def _entries(lists, cap, stride, offset, n_lists, F):
    L = np.asarray(lists, dtype=I32).reshape(-1)[:n_lists * stride].reshape(n_lists, stride)
    return L[:, offset:offset + cap * (1 + F)].reshape(n_lists, cap, 1 + F)


def in_range_rows(entries, total_rows):
    """per list: the rows a kernel may touch"""
    return [e[(e[:, 0] >= 0) & (e[:, 0] < total_rows), 0] for e in entries]


def apply_ref(dense, lists, cap, stride, offset, n_lists, scale, total_rows):
    """hm_rows_apply: list after list, dst = fl(dst + fl(v * fl(scale))) - two separately rounded fp32 operations"""
    out = dense.astype(F32, copy=True)
    F = out.shape[1]
    s = F32(scale)
    if cap == 0 or n_lists == 0:
        return out
    for e in _entries(lists, cap, stride, offset, n_lists, F):
        ok = (e[:, 0] >= 0) & (e[:, 0] < total_rows)
        rows = e[ok, 0]
        assert np.unique(rows).size == rows.size, "rows must be unique inside a list"
        v = np.ascontiguousarray(e[ok, 1:]).view(F32)
        prod = np.multiply(v, s, dtype=F32)
        out[rows] = np.add(out[rows], prod, dtype=F32)
    return out


def clear_ref(dense, lists, cap, stride, offset, n_lists, total_rows, count=None):
    """hm_rows_clear: (dense after, counter after).  Exactly the in-range rows named by the lists become +0.0"""
    out = dense.astype(F32, copy=True)
    F = out.shape[1]
    if cap and n_lists:
        for rows in in_range_rows(_entries(lists, cap, stride, offset, n_lists, F), total_rows):
            out[rows] = 0.0
    return out, (None if count is None else 0)


# ---- the host protocol as a simulated world of three -----------------------------------------------------------------
WORLD = 3
WORLD_GRID = dict(n_levels=4, n_features=2, log2_hashmap_size=10, base_resolution=4, desired_resolution=32)
WORLD_POINTS = 500                  # per rank: a static step has the same count everywhere
WORLD_MAX_ABS = 8.0


def world_inputs(rank):
    """(x [n, 3], d_feat [n, L * F]) of one rank.  d_feat holds multiples of 2^-6 of magnitude <= 8 and the reference
    weights are 0 / 1, so every partial sum of a row (< 500 * 8) is exact in fp32 in ANY order: the atomic scatters of
    two rounds, and of ops.encode_bwd_table, give the same bits.  A fifth of the points repeat, so rows collect several
    contributions; the ranks share some points, so rows appear in several payloads"""
    rs = np.random.RandomState(300 + rank)
    n, g = WORLD_POINTS, WORLD_GRID
    x = rs.uniform(-1.1, 1.1, (n, 3)).astype(F32)
    x[n - n // 5:] = x[:n // 5]
    x[:40] = np.random.RandomState(299).uniform(-1.0, 1.0, (40, 3)).astype(F32)          # the same on every rank
    d = rs.randint(-512, 513, (n, g["n_levels"] * g["n_features"])).astype(F32) / F32(64.0)
    return x, d


# ---- hm_multi_copy_f32 -----------------------------------------------------------------------------------------------
COPY_MAX_ITEMS = 96                 # HM_COPY_MAX_ITEMS of include/hashmod.h
COPY_CHUNK = 8192                   # floats per workgroup
# (numel, source float offset, destination float offset); an offset that is a multiple of 4 is 16-byte aligned
COPY_ITEMS = [
    (1, 0, 0), (3, 0, 0), (4, 0, 0), (6, 0, 0), (8191, 0, 0), (0, 0, 0), (8192, 0, 0), (8193, 0, 0), (8194, 0, 0),
    (8195, 0, 0), (16385, 0, 0), (0, 0, 0),                          # the float4 body and its tail, numel % 4 = 0 .. 3
    (4, 1, 0), (8193, 2, 0), (16385, 3, 0),                          # misaligned source into an aligned destination
    (4, 0, 1), (8195, 0, 3), (8191, 0, 2),                           # aligned source, misaligned destination
    (1, 1, 1), (3, 3, 2), (8192, 1, 1), (0, 0, 0), (16385, 2, 3),    # both misaligned (equal and unequal offsets)
    (512 * 512 + 3, 0, 0), (512 * 512 + 3, 0, 1),                    # many chunks, both paths
]
COPY_MANY = [((0, 0, 0) if i % 17 == 5 else (1 + (7 * i) % 13, i % 4 if i % 3 == 0 else 0, (i // 2) % 4 if i % 5 else 0))
             for i in range(213)]         # 200 live items (three tables of at most 96) and 13 empty ones
COPY_PAD = 4                        # floats after every source and after the last window (fill: COPY_SRC_PAD / sentinel)
COPY_SENTINEL = F32(-12345.5)
COPY_SRC_PAD = F32(777.25)


def copy_class(item):
    """(source aligned, destination aligned)"""
    return item[1] % 4 == 0, item[2] % 4 == 0


def copy_sources(items, seed=0):
    """one float32 array per item: values no window of the bucket holds before the call (never the sentinel)"""
    rs = np.random.RandomState(9 + seed)
    return [(rs.standard_normal(n).astype(F32) + F32(3.0) * F32(k + 1)) for k, (n, _, _) in enumerate(items)]


def copy_layout(items):
    """(window start per item, bucket size): windows in item order, each at the first position that leaves at least one
    guard float after the previous window and has the item's destination offset modulo 4; zero-numel items get none"""
    starts, pos = [], 1
    for n, _, d in items:
        if n == 0:
            starts.append(None)
            continue
        pos += (d - pos) % 4
        starts.append(pos)
        pos += n + 1
    return starts, pos + COPY_PAD


def copy_ref(items, sources):
    """hm_multi_copy_f32 on a bucket filled with COPY_SENTINEL"""
    starts, size = copy_layout(items)
    flat = np.full(size, COPY_SENTINEL, dtype=F32)
    for (n, _, _), s, src in zip(items, starts, sources):
        if n:
            flat[s:s + n] = src
    return flat
