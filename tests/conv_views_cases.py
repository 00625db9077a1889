"""Cases for the forward fp32 convolution (fpcc_conv_f32 / fpcc_conv_f32_pk, fpcc_conv_k2s2t_f32, fpcc_gather_sum*_f32) on operands
that are VIEWS: plain operands derived from one small scene, the oracle's expected output, and the recipe that wraps an operand into
a hostile view.  NumPy and the oracle only -- no GPU; test_conv_views_cases.py checks on the CPU that the views hold what they promise
and that their poison bites, test_gpu_conv_views.py runs every kernel form on them.

Scene: surface_cloud(SEED, 32, 1500) -> a fine level (1108 rows) cut to N_FINE = n - 13 rows and its stride-2 level (617 rows) cut to
N_COARSE = m - 21 rows; both counts are ragged for 32- and for 64-row units.  Table entries that point past a cut are -1, so the cut
leaves fine rows no coarse row lists (the transposed kinds skip them).

Kinds (n_offsets, groups):
    k3     27, 1   fine -> fine through the 3x3x3 table [27, N_FINE]
    k2s2    8, 1   fine -> coarse through the 2x2x2 table [8, N_COARSE] (child_row transposed)
    pw      1, 1   per point on the fine level, identity map
    k2s2T   1, 8   coarse -> fine through out_map = child_row [N_COARSE, 8]; N_FINE + EXTRA_OUT_ROWS output rows, the unlisted ones skipped
    gen     1, 8   coarse -> all eight children, row 8 * parent + octant

Input view (Frame): big[G_TOP : G_TOP + rows, off : off + c] of a buffer with G_TOP guard rows above, G_BOTTOM below and a pitch of
c + PAD['x1' | 'x2']; off = OFF_ALIGNED (16 bytes) or OFF_MISALIGNED (4 bytes).  Beside a table the view has a SPARE row 0 in front of
the data and every table entry >= 0 is shifted by + 1 (shifted()): no entry names row 0, so a kernel that clamps -1 to row 0 reads
poison.  Every cell outside the data is a quiet NaN.  Weights and bias stay finite (the precondition of fpcc_conv_f32_pk).
Output view: the same frame without a spare row, the whole buffer filled with the NaN SENTINEL beforehand; compared as int32.

Tables are handed over as contiguous 1-D int32 slices, (nbr_ks, nbr_os) carry the shape:
    plain     offset-major [K, n]                                  (n, 1)
    wide      offset-major, pitch n + 7, 4-byte pointer offset      (n + 7, 1), flat[3:]; the padding names row 0 (poison under a shift)
    rows      row-major [n, ld], ld = 32 | 8, padding -1            (1, ld): what fpcc_transpose_table_i32 writes
    rows_pos  rows gathered into position order beside a row order  (1, ld): what fpcc_gather_table_rows_i32 writes
    rows27    row-major [n, K] without padding                      (1, K): NOT a table the kernels read by position
    rows_off1 `rows` 4 bytes into its buffer                        (1, ld), flat[1:]: neither
"""
import functools
from collections import namedtuple

import numpy as np

from oracle import coords as oc
from oracle import sparse_conv as sc
from util import batched, surface_cloud

SEED = 41
CUT_FINE, CUT_COARSE = 13, 21
EXTRA_OUT_ROWS = 4                     # output rows of the transposed kind past the fine level: no parent lists them
G_TOP, G_BOTTOM = 3, 5
PAD = {'x1': 12, 'x2': 20, 'out': 12, 'y': 12}
OFF_ALIGNED, OFF_MISALIGNED = 4, 1
SENTINEL = 0x7FC12345                  # a quiet NaN with a payload no kernel produces
SLOPE, CLIP = 0.2, 1.5

N_OFF = {'k3': 27, 'k2s2': 8, 'pw': 1, 'k2s2T': 1, 'gen': 1}
GROUPS = {'k3': 1, 'k2s2': 1, 'pw': 1, 'k2s2T': 8, 'gen': 8}

Scene = namedtuple('Scene', 'n_fine n_coarse k3 k2 child_row parent_nbr gen_table')
Case = namedtuple('Case', 'kind c1 c2 c_out n_in n_out out_rows n_off groups x1 x2 w bias table out_map')
Frame = namedtuple('Frame', 'rows_total pitch r0 rows off c spare')


def _frozen(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def scene() -> Scene:
    lvl = oc.Level(batched(surface_cloud(SEED, 32, 1500)), 1)
    up = oc.strided(lvl)
    n, m = lvl.n - CUT_FINE, up.n - CUT_COARSE
    k3 = oc.dense_table(oc.kernel_map(lvl, lvl, 3), lvl.n)[:, :n].astype(np.int32)
    k3[k3 >= n] = -1
    k2 = oc.dense_table(oc.kernel_map(lvl, up, 2), up.n)[:, :m].astype(np.int32)
    k2[k2 >= n] = -1
    child_row = np.ascontiguousarray(k2.T)
    # the coarse level's own 3x3x3 table (uncut: gather_sum_generated takes the parents' table) and the table of its generated set
    parent_nbr = oc.dense_table(oc.kernel_map(up, up, 3), up.n).astype(np.int32)
    gen = oc.generated(up)
    gen_table = oc.dense_table(oc.kernel_map(gen, gen, 3), gen.n).astype(np.int32)
    _frozen(k3, k2, child_row, parent_nbr, gen_table)
    return Scene(n, m, k3, k2, child_row, parent_nbr, gen_table)


@functools.lru_cache(maxsize=None)
def case(kind: str, c1: int, c2: int, c_out: int) -> Case:
    """plain operands of one shape (read-only, shared)"""
    s = scene()
    k, g = N_OFF[kind], GROUPS[kind]
    rng = np.random.default_rng([sorted(N_OFF).index(kind), c1, c2, c_out])
    table = out_map = out_rows = None
    if kind == 'k3':
        n_in = n_out = s.n_fine
        table = s.k3
    elif kind == 'k2s2':
        n_in, n_out, table = s.n_fine, s.n_coarse, s.k2
    elif kind == 'pw':
        n_in = n_out = s.n_fine
    else:
        n_in = n_out = s.n_coarse
        if kind == 'k2s2T':
            out_map, out_rows = s.child_row, s.n_fine + EXTRA_OUT_ROWS
    if out_rows is None:
        out_rows = n_out * g
    c_in = c1 + c2
    x1 = rng.normal(size=(n_in, c1)).astype(np.float32)
    x2 = rng.normal(size=(n_in, c2)).astype(np.float32) if c2 else None
    w = (rng.normal(size=(g * k, c_in, c_out)) / np.sqrt(max(1, k // 2) * c_in)).astype(np.float32)
    bias = rng.normal(size=c_out).astype(np.float32)
    _frozen(x1, x2, w, bias)
    return Case(kind, c1, c2, c_out, n_in, n_out, out_rows, k, g, x1, x2, w, bias, table, out_map)


def chain(c: Case, order: int, x1=None, x2=None, table=None):
    """the oracle's chain of summation order `order` -> (out [out_rows, c_out], written [out_rows] bool); x1, x2, table: operands in
    place of the case's own (views, shifted tables)"""
    x1 = c.x1 if x1 is None else x1
    x2 = c.x2 if x2 is None else x2
    table = c.table if table is None else table
    kw = dict(act=sc.ACT_PRELU, slope=SLOPE, clip=CLIP, order=order)
    if c.groups == 1:
        return sc.conv_chain(x1, table, c.w, c.bias, c.n_out, x2=x2, **kw), np.ones(c.out_rows, bool)
    out = np.zeros((c.out_rows, c.c_out), np.float32)
    written = np.zeros(c.out_rows, bool)
    for g in range(8):
        y = sc.conv_chain(x1, None, c.w[g], c.bias, c.n_out, x2=x2, **kw)
        if c.out_map is not None:
            rows = c.out_map[:, g]
            out[rows[rows >= 0]] = y[rows >= 0]
            written[rows[rows >= 0]] = True
        else:
            out[g::8] = y
            written[g::8] = True
    return out, written


@functools.lru_cache(maxsize=None)
def expected(kind: str, c1: int, c2: int, c_out: int, order: int):
    out, written = chain(case(kind, c1, c2, c_out), order)
    _frozen(out, written)
    return out, written


# ---- views ----------------------------------------------------------------------------------------------------------------------------
def frame(rows: int, c: int, off: int, pad: int, spare: bool = False) -> Frame:
    """the view big[r0 : r0 + rows (+ 1 with a spare row), off : off + c] of a [rows_total, pitch] buffer"""
    rows += int(spare)
    return Frame(G_TOP + rows + G_BOTTOM, c + pad, G_TOP, rows, off, c, spare)


def input_frame(name: str, c: Case, off: int = OFF_ALIGNED, pad=None) -> Frame:
    return frame(c.n_in, c.c1 if name == 'x1' else c.c2, off, PAD[name] if pad is None else pad, spare=c.table is not None)


def output_frame(c: Case, off: int = OFF_ALIGNED, pad=None) -> Frame:
    return frame(c.out_rows, c.c_out, off, PAD['out'] if pad is None else pad)


def view(big, f: Frame):
    """the frame's view of its buffer (a NumPy array or a torch tensor [rows_total, pitch])"""
    return big[f.r0:f.r0 + f.rows, f.off:f.off + f.c]


def poisoned(f: Frame, x: np.ndarray) -> np.ndarray:
    """float32 [rows_total, pitch]: NaN everywhere but the data x, which sits behind the spare row if the frame has one"""
    big = np.full((f.rows_total, f.pitch), np.nan, np.float32)
    view(big, f)[int(f.spare):] = x
    return big


def sentinel(f: Frame) -> np.ndarray:
    """int32 [rows_total, pitch] full of SENTINEL: the output buffer before a launch"""
    return np.full((f.rows_total, f.pitch), SENTINEL, np.int32)


def expected_buffer(f: Frame, out: np.ndarray, written: np.ndarray) -> np.ndarray:
    """int32 image of the output buffer after a launch: the written rows of `out` inside the view, SENTINEL in every other cell"""
    big = sentinel(f)
    v = view(big, f)
    v[written] = np.ascontiguousarray(out).view(np.int32)[written]
    return big


def plain_input(x: np.ndarray, spare: bool) -> np.ndarray:
    """the contiguous operand that goes with a shifted table: x behind one NaN row"""
    return np.concatenate((np.full((1, x.shape[1]), np.nan, np.float32), x)) if spare else x


def shifted(table: np.ndarray) -> np.ndarray:
    """entries >= 0 moved past the spare row 0"""
    return np.where(table >= 0, table + 1, -1).astype(np.int32)


@functools.lru_cache(maxsize=None)
def row_order(n: int) -> np.ndarray:
    """a fixed permutation of the n output rows"""
    p = np.random.default_rng(n).permutation(n).astype(np.int32)
    _frozen(p)
    return p


TABLES = ('plain', 'wide', 'rows', 'rows_pos', 'rows27', 'rows_off1')
Table = namedtuple('Table', 'flat ks os by_position qualifies lead')


def rows_ld(k: int) -> int:
    return 8 if k == 8 else 32


def table_variant(table: np.ndarray, variant: str, order=None) -> Table:
    """-> contiguous int32 slice, (nbr_ks, nbr_os), whether its rows are in position order (`order` given), whether beside a row
    order the library reads it by position (aligned 16-byte pieces) -- rows27 and rows_off1 do not --, and lead: the int32 words in
    front of the slice in its buffer (a device copy must keep them: they are the pointer's misalignment)"""
    k, n = table.shape
    table = table.astype(np.int32)
    if variant == 'plain':
        return Table(np.ascontiguousarray(table).reshape(-1), n, 1, False, True, 0)
    if variant == 'wide':
        buf = np.zeros(3 + k * (n + 7), np.int32)                       # padding: row 0, the spare row of a shifted table
        flat = buf[3:]
        flat.reshape(k, n + 7)[:, :n] = table
        return Table(flat, n + 7, 1, False, True, 3)
    if variant not in TABLES:
        raise ValueError(variant)
    ld = k if variant == 'rows27' else rows_ld(k)
    rows = np.full((n, ld), -1, np.int32)
    rows[:, :k] = table.T
    by_position = order is not None and variant != 'rows'
    if variant == 'rows_pos' and order is None:
        raise ValueError('rows_pos goes with a row order')
    if by_position:
        rows = rows[order]
    if variant == 'rows_off1':
        buf = np.full(1 + n * ld, -1, np.int32)
        buf[1:] = rows.reshape(-1)
        return Table(buf[1:], 1, ld, by_position, False, 1)
    return Table(np.ascontiguousarray(rows).reshape(-1), 1, ld, by_position, ld % 4 == 0, 0)


# ---- deliberately wrong host-side evaluations: what the poison is there to catch ----------------------------------------------------
def chain_clamping_absent_to_row_0(c: Case, order: int, x1v: np.ndarray, x2v, table: np.ndarray) -> np.ndarray:
    """a kernel that reads row 0 for an absent neighbour and relies on the product being dropped"""
    return chain(c, order, x1=x1v, x2=x2v, table=np.maximum(table, 0))[0]


def view_with_pitch_c(big: np.ndarray, f: Frame) -> np.ndarray:
    """a kernel that steps from row to row by the row's width c instead of the pitch: same origin, wrong rows"""
    flat = big.reshape(-1)[f.r0 * f.pitch + f.off:]
    return np.lib.stride_tricks.as_strided(flat, (f.rows, f.c), (4 * f.c, 4))


# ---- the one-output-channel gather (fpcc_gather_sum_f32, fpcc_gather_sum_generated_f32) ------------------------------------------------
def gather_sum_chain(y: np.ndarray, table: np.ndarray, bias: float) -> np.ndarray:
    """out[o] = act(sum_k y[table[k, o], k] + bias): the partial sums added in ascending offset order in fp32 (order 2's second half)"""
    k, n = table.shape
    acc = np.zeros(n, np.float32)
    for j in range(k):
        idx = table[j]
        acc = np.where(idx >= 0, (acc + y[np.maximum(idx, 0), j]).astype(np.float32), acc)
    v = (acc + np.float32(bias)).astype(np.float32)
    v = np.where(v < 0, (v * np.float32(SLOPE)).astype(np.float32), v)
    return np.clip(v, -np.float32(CLIP), np.float32(CLIP)).astype(np.float32).reshape(n, 1)


@functools.lru_cache(maxsize=None)
def gather_case(generated: bool):
    """-> (y [rows, 27], table [27, n], bias, expected [n, 1]); generated: the 8 candidates per coarse row, table from the oracle's
    generated level -- the kernel derives it from scene().parent_nbr"""
    s = scene()
    table = s.gen_table if generated else s.k3
    rows = table.shape[1] if generated else s.n_fine
    rng = np.random.default_rng(77 + generated)
    y = rng.normal(size=(rows, 27)).astype(np.float32)
    want = gather_sum_chain(y, table, 0.37)
    _frozen(y, want)
    return y, table, 0.37, want
