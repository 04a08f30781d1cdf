"""The exact text and code of every refusal of the Rainbow population's entry points, in the style of
tests/test_rainbow_learn_refusal_texts.py: the argument checks run before any launch or read, so fake,
never-dereferenced pointers drive them on a host without a GPU. A row with two bad arguments pins which check
fires first; a refusal of one member's fields names the member."""
import ctypes

import numpy as np
import pytest

FAKE = 1 << 20          # 16-byte aligned
ODD8 = (1 << 20) + 8    # 8-byte aligned only
ODD4 = (1 << 20) + 4
ODD2 = (1 << 20) + 2

DEV, HOST, INIT = "mg_rainbow_learn_many", "mg_host_rainbow_learn_many", "mg_rainbow_learn_many_init"
NOISE, HNOISE, SYNC = "mg_rainbow_noise_many", "mg_host_rainbow_noise_many", "mg_rainbow_sync_target_many"


def texts(what):
    w = what.encode()
    return dict(
        members=w + b": need 1 <= members <= 64", null=w + b": NULL pointer",
        mnull=lambda m: w + b": member %d: NULL pointer (rows or counter)" % m,
        batch=w + b": need 1 <= batch <= 1024", cap=w + b": need 1 <= capacity <= 2^32", neg=w + b": num_updates < 0",
        noise=w + b": noise is NULL (num_updates x members x 2 x 1124 factors)",
        beta=lambda m: w + b": member %d: need 0 <= beta1 < 1 and 0 <= beta2 < 1" % m,
        align=w + b": learners, scratch and packed_out must be 16-byte, noise and the optional outputs 4-byte "
                  b"aligned, packed_stride a multiple of 16",
        malign=lambda m: w + b": member %d: rows and counter must be 8-byte aligned" % m,
        stride=w + b": packed_stride smaller than mg_rainbow_packed_bytes()",
        scratch=w + b": scratch smaller than members * mg_rainbow_learn_scratch_bytes(batch)",
        tnull=w + b": table is NULL", talign=w + b": table must be 16-byte aligned",
        tsize=w + b": table smaller than mg_rainbow_learn_many_table_bytes(members)")


def learn_rows(what, device):
    t = texts(what)
    rows = [
        ("members 0", dict(members=0), t["members"]),
        ("members 65", dict(members=65), t["members"]),
        ("learners NULL", dict(learners=None), t["null"]),
        ("member NULL", dict(no_member=True), t["null"]),
        ("scratch NULL", dict(scratch=None), t["null"]),
        ("member 1 rows NULL", dict(member={1: dict(rows=None)}), t["mnull"](1)),
        ("member 2 counter NULL", dict(member={2: dict(counter=None)}), t["mnull"](2)),
        ("batch 0", dict(batch=0), t["batch"]),
        ("batch 1025", dict(batch=1025), t["batch"]),
        ("capacity 0", dict(capacity=0), t["cap"]),
        ("capacity 2^32 + 1", dict(capacity=(1 << 32) + 1), t["cap"]),
        ("num_updates -1", dict(num_updates=-1), t["neg"]),
        ("noise NULL", dict(noise=None), t["noise"]),
        ("member 0 beta1 1", dict(member={0: dict(beta1=1.0)}), t["beta"](0)),
        ("member 2 beta2 -0.1", dict(member={2: dict(beta2=-0.1)}), t["beta"](2)),
        ("learners misaligned", dict(learners=ODD8), t["align"]),
        ("scratch misaligned", dict(scratch=ODD8), t["align"]),
        ("noise misaligned", dict(noise=ODD2), t["align"]),
        ("loss_out misaligned", dict(loss_out=ODD2), t["align"]),
        ("rows_out misaligned", dict(rows_out=ODD2), t["align"]),
        ("proj_out misaligned", dict(proj_out=ODD2), t["align"]),
        ("grads_out misaligned", dict(grads_out=ODD2), t["align"]),
        ("member 1 rows misaligned", dict(member={1: dict(rows=ODD4)}), t["malign"](1)),
        ("member 0 counter misaligned", dict(member={0: dict(counter=ODD4)}), t["malign"](0)),
        ("scratch one byte short", dict(scratch_short=1), t["scratch"]),
        # the order, one pair of adjacent checks each
        ("members before NULL", dict(members=65, learners=None), t["members"]),
        ("NULL before a member's NULL", dict(scratch=None, member={0: dict(rows=None)}), t["null"]),
        ("a member's NULL before batch", dict(member={1: dict(rows=None)}, batch=0), t["mnull"](1)),
        ("batch before capacity", dict(batch=0, capacity=0), t["batch"]),
        ("capacity before num_updates", dict(capacity=0, num_updates=-1), t["cap"]),
        ("num_updates before noise", dict(num_updates=-1, noise=None), t["neg"]),
        ("noise before beta", dict(noise=None, member={0: dict(beta1=2.0)}), t["noise"]),
        ("beta before alignment", dict(member={1: dict(beta2=1.0)}, learners=ODD8), t["beta"](1)),
        ("alignment before a member's", dict(loss_out=ODD2, member={0: dict(rows=ODD4)}), t["align"]),
        ("a member's alignment before scratch size", dict(member={2: dict(counter=ODD4)}, scratch_short=8),
         t["malign"](2)),
        ("the lowest member is named", dict(member={1: dict(beta1=1.0), 2: dict(beta1=1.0)}), t["beta"](1)),
    ]
    if device:
        rows += [
            ("packed_out misaligned", dict(packed_out=ODD8), t["align"]),
            ("packed_stride 74200", dict(packed_stride=74200), t["align"]),
            ("packed_stride short", dict(packed_stride=74192 - 16), t["stride"]),
            ("table NULL", dict(table=None), t["tnull"]),
            ("table misaligned", dict(table=ODD8), t["talign"]),
            ("table one byte short", dict(table_short=1), t["tsize"]),
            ("a member's alignment before packed_stride", dict(member={0: dict(rows=ODD4)}, packed_stride=16),
             t["malign"](0)),
            ("packed_stride before scratch size", dict(packed_stride=16, scratch_short=8), t["stride"]),
            ("scratch size before table", dict(scratch_short=8, table=None), t["scratch"]),
            ("table NULL before its size", dict(table=None, table_short=8), t["tnull"]),
            ("table alignment before its size", dict(table=ODD8, table_short=8), t["talign"]),
        ]
    return [(what, *r) for r in rows]


def init_rows():
    t = texts(INIT)
    return [(INIT, *r) for r in [
        ("members 0", dict(members=0), t["members"]),
        ("members 65", dict(members=65), t["members"]),
        ("member NULL", dict(no_member=True), t["null"]),
        ("member 1 rows NULL", dict(member={1: dict(rows=None)}), t["mnull"](1)),
        ("member 0 beta2 1", dict(member={0: dict(beta2=1.0)}), t["beta"](0)),
        ("member 2 rows misaligned", dict(member={2: dict(rows=ODD4)}), t["malign"](2)),
        ("table NULL", dict(table=None), t["tnull"]),
        ("table misaligned", dict(table=ODD8), t["talign"]),
        ("table one byte short", dict(table_short=1), t["tsize"]),
        ("members before member NULL", dict(members=0, no_member=True), t["members"]),
        ("NULL before beta", dict(member={2: dict(rows=None), 0: dict(beta1=1.0)}), t["mnull"](2)),
        ("beta before alignment", dict(member={2: dict(beta1=1.0), 0: dict(rows=ODD4)}), t["beta"](2)),
        ("alignment before table", dict(member={1: dict(counter=ODD4)}, table=None), t["malign"](1)),
        ("table NULL before its size", dict(table=None, table_short=8), t["tnull"]),
        ("table alignment before its size", dict(table=ODD8, table_short=8), t["talign"]),
    ]]


def noise_rows(what):
    w = what.encode()
    return [(what, *r) for r in [
        ("members 0", dict(members=0), w + b": need 1 <= members <= 64"),
        ("members 65", dict(members=65), w + b": need 1 <= members <= 64"),
        ("noise_seed NULL", dict(noise_seed=None), w + b": NULL pointer"),
        ("first_update NULL", dict(first_update=None), w + b": NULL pointer"),
        ("noise_out NULL", dict(noise_out=None), w + b": NULL pointer"),
        ("num_updates -1", dict(num_updates=-1), w + b": num_updates < 0"),
        ("noise_out misaligned", dict(noise_out=ODD2), w + b": noise_out must be 4-byte aligned"),
        ("past the grid", dict(num_updates=(1 << 31) - 1, members=64), w + b": num_updates * members exceeds the grid limit"),
        ("members before NULL", dict(members=0, noise_out=None), w + b": need 1 <= members <= 64"),
        ("NULL before num_updates", dict(noise_out=None, num_updates=-1), w + b": NULL pointer"),
        ("num_updates before alignment", dict(num_updates=-1, noise_out=ODD2), w + b": num_updates < 0"),
        ("alignment before the grid", dict(noise_out=ODD2, num_updates=(1 << 31) - 1, members=64),
         w + b": noise_out must be 4-byte aligned"),
    ]]


SYNC_ROWS = [(SYNC, *r) for r in [
    ("members 0", dict(members=0), b"mg_rainbow_sync_target_many: need 1 <= members <= 64"),
    ("members 65", dict(members=65), b"mg_rainbow_sync_target_many: need 1 <= members <= 64"),
    ("learners NULL", dict(learners=None), b"mg_rainbow_sync_target_many: NULL pointer"),
    ("learners misaligned", dict(learners=ODD8), b"mg_rainbow_sync_target_many: learners must be 16-byte aligned"),
    ("bit 3 of 3 members", dict(mask=0b1000), b"mg_rainbow_sync_target_many: mask has a bit at or above members"),
    ("members before NULL", dict(members=0, learners=None), b"mg_rainbow_sync_target_many: need 1 <= members <= 64"),
    ("NULL before the mask", dict(learners=None, mask=0b1000), b"mg_rainbow_sync_target_many: NULL pointer"),
    ("alignment before the mask", dict(learners=ODD8, mask=0b1000),
     b"mg_rainbow_sync_target_many: learners must be 16-byte aligned"),
]]

TABLE = (learn_rows(DEV, True) + learn_rows(HOST, False) + init_rows() + noise_rows(NOISE) + noise_rows(HNOISE)
         + SYNC_ROWS)


def _ptr(v):
    return None if v is None else ctypes.c_void_p(v)


def _members(count, over):
    from merging_gym import _native

    arr = (_native.DqnMember * max(count, 1))()
    for m in range(max(count, 1)):
        f = dict(rows=FAKE, counter=FAKE, beta1=0.9, beta2=0.999)
        f.update(over.get(m, {}))
        arr[m] = _native.DqnMember(f["rows"], f["counter"], m, 0, 0,
                                   _native.DqnHyper(0.001, 0.99, f["beta1"], f["beta2"], 1e-8, 1, 0))
    return arr


def _call(entry, over):
    """Call `entry` with arguments that pass every check, except for `over`; (return value, error text, members)."""
    from merging_gym import _native

    lib = _native.lib
    a = dict(over)
    g = a.pop
    M = g("members", 3)
    members = None
    if entry in (DEV, HOST, INIT):
        members = _members(min(M, 64), g("member", {}))
        mp = None if g("no_member", False) else members
        table = [_ptr(g("table", FAKE)), lib.mg_rainbow_learn_many_table_bytes(3) - g("table_short", 0)]
    if entry == INIT:
        args = table + [mp, M, None]
    elif entry in (DEV, HOST):
        nbytes = 3 * lib.mg_rainbow_learn_scratch_bytes(32) - g("scratch_short", 0)
        args = [_ptr(g("learners", FAKE))] + (table if entry == DEV else []) + [
            mp, M, g("capacity", 100), g("batch", 32), g("num_updates", 1), _ptr(g("noise", FAKE)),
            _ptr(g("loss_out", FAKE)), _ptr(g("rows_out", FAKE)), _ptr(g("proj_out", FAKE)), _ptr(g("grads_out", FAKE))]
        if entry == DEV:
            args += [_ptr(g("packed_out", FAKE)), g("packed_stride", 74192)]
        args += [_ptr(g("scratch", FAKE)), nbytes] + ([None] if entry == DEV else [])
    elif entry in (NOISE, HNOISE):
        args = [_ptr(g("noise_seed", FAKE)), _ptr(g("first_update", FAKE)), M, g("num_updates", 1),
                _ptr(g("noise_out", FAKE))] + ([None] if entry == NOISE else [])
    elif entry == SYNC:
        args = [_ptr(g("learners", FAKE)), M, g("mask", 0b101), None]
    assert not a, f"unknown overrides {a}"
    rc = getattr(lib, entry)(*args)
    return rc, lib.mg_last_error(), members


@pytest.mark.parametrize("entry,case,over,text", TABLE, ids=[f"{r[0]}-{r[1]}" for r in TABLE])
def test_refusal(entry, case, over, text):
    rc, got, members = _call(entry, over)
    assert (rc, got) == (1, text)
    for e in members or ():  # a refused call leaves the counters
        assert (int(e.first_update), int(e.first_draw)) == (0, 0)


def test_sizes_and_the_member_limits():
    from merging_gym import _native

    lib = _native.lib
    assert [lib.mg_rainbow_learn_many_table_bytes(m) for m in (0, 1, 64, 65)] == [0, 48, 64 * 48, 0]
    assert lib.mg_rainbow_packed_bytes() == 74192
    assert lib.mg_abi_version() == 21  # the entry points are additive


def test_members_1_and_64_pass_the_host_checks():
    """On real (host) memory: one member and 64 members learn; num_updates == 0 is the lone learner's no-op -- the
    effective weights of the stored noise into the scratch, nothing else (the device call then packs) -- and
    moves no counter."""
    import rainbow_learn_many_ref as many

    for M in (1, 64):
        settings, ring_list = many.member_settings(M), many.rings(M)
        L = many.learners(M)
        got = many.run_host_members(L, settings, ring_list, 1, 1, many.noise(1, M))
        assert np.isfinite(got[1]).all() and got[1].shape == (1, M)
        assert [int(e.first_update) for e in got[5]] == [s["first_update"] + 1 for s in settings]
        none = many.run_host_members(L, settings, ring_list, 1, 0, np.zeros((0, M, 2, many.NF), np.float32))
        assert (none[0].view(np.uint32) == L.view(np.uint32)).all()
        assert [int(e.first_update) for e in none[5]] == [s["first_update"] for s in settings]
