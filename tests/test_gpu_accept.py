"""Client acceptance on the GPU: pbft_wire_decode_replies_device, pbft_accept_replies_device and pbft_accept_replies
against the Python model (pbft_amd.accept_reference with the C oracle's verify_strict, tests/accept_sim.py) and, reply
by reply, against pbft_wire_decode_reply, hashlib and pbft_records_pack -- over poisoned outputs with guards in front of
and behind every buffer; then a capture and replay, the library's own signer end to end, the arguments and a key change."""
import hashlib

import numpy as np
import pytest

import accept_sim as A
from pbft_amd import wire

pytestmark = pytest.mark.gpu
POISON, GUARD = 0xA5, 512
NONE = wire.ACCEPT_NO_REPLY


@pytest.fixture(scope="module")
def av():
    """A verifier with the four replicas' keys and their PeerId table."""
    from pbft_amd import GpuBatchVerifier
    v = GpuBatchVerifier(0)
    assert v.set_keys(A.world().keys).all()
    v.accept_reserve(512)
    v.reserve(512)
    v.group_reserve(512)
    yield v
    v.close()


def guarded(torch, dev, size):
    t = torch.full((GUARD + size + GUARD,), POISON, dtype=torch.uint8, device=dev)
    assert t.data_ptr() % 16 == 0
    return t


def body(t, size):
    a = t.cpu().numpy()
    assert (a[:GUARD] == POISON).all(), "bytes in front of an output overwritten"
    assert (a[GUARD + size:] == POISON).all(), "bytes behind an output overwritten"
    return a[GUARD:GUARD + size].copy()


def clients_table():
    return np.frombuffer(b"".join(wire.client_field(c) for c in A.CLIENTS), np.uint8).copy()


def run_device(v, packed, client_idx, env_cap=None, chain=True, need=A.NEED, n_clients=len(A.CLIENTS)):
    """One device call over poisoned outputs -> dict of everything it wrote, every guard checked."""
    import torch
    dev = torch.device("cuda", 0)
    buf, off, lens, text_bytes = packed
    n = len(off)
    cap = max(n, 1) if env_cap is None else env_cap
    W = (v.n_keys + 63) // 64
    ins = [torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy() if a.size else
                            np.zeros(16, np.uint8)).to(dev) for a in (buf, off, lens, client_idx, clients_table())]
    p = [t.data_ptr() for t in ins]
    assert p[0] % 16 == 0
    sizes = dict(records=160 * n, heads=32 * n, bitmap=8 * ((n + 63) // 64), env_idx=4 * n, envelopes=85 * cap, n_env=8,
                 signers=8 * cap * W, counts=4 * cap, certs=32 * cap)
    d = {k: guarded(torch, dev, s) for k, s in sizes.items()}
    q = {k: t.data_ptr() + GUARD for k, t in d.items()}
    s = torch.cuda.Stream()
    if chain:
        v.accept_replies_device(p[0], text_bytes, p[1], p[2], p[4], n_clients, n, need, q["records"], q["heads"],
                                q["bitmap"], cap, q["env_idx"], q["envelopes"], q["n_env"], q["signers"], q["counts"],
                                q["certs"], d_client_idx=p[3], stream=s.cuda_stream)
    else:
        v.decode_replies_device(p[0], text_bytes, p[1], p[2], p[4], n_clients, n, q["records"], q["heads"],
                                d_client_idx=p[3], stream=s.cuda_stream)
    s.synchronize()
    raw = {k: body(t, sizes[k]) for k, t in d.items()}
    out = dict(records=raw["records"].reshape(n, 160), heads=raw["heads"].view(wire.AcceptHead))
    if chain:
        out.update(bits=np.unpackbits(raw["bitmap"], bitorder="little")[:n].astype(bool),
                   env_idx=raw["env_idx"].view(np.uint32), envelopes=raw["envelopes"].reshape(cap, 85),
                   n_env=raw["n_env"].view(np.uint32), signers=raw["signers"].view(np.uint64).reshape(cap, W),
                   counts=raw["counts"].view(np.uint32), certs=raw["certs"].view(wire.AcceptCert))
    else:
        for k in ("bitmap", "env_idx", "envelopes", "n_env", "signers", "counts", "certs"):
            assert (raw[k] == POISON).all(), k
    return out


def first_bad(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    if len(a) == 0:
        return []
    if a.dtype.names:
        a, b = a.view(np.uint8).reshape(len(a), -1), b.view(np.uint8).reshape(len(b), -1)
    bad = np.nonzero((a != b).reshape(len(a), -1).any(axis=1))[0] if len(a) else np.zeros(0, int)
    return list(bad[:8])


def check_decode(got, m, c):
    assert not first_bad(got["heads"], m["heads"]), (first_bad(got["heads"], m["heads"]),
                                                     [c["note"][i] for i in first_bad(got["heads"], m["heads"])])
    want = A.records_of(m)
    assert not first_bad(got["records"], want), [c["note"][i] for i in first_bad(got["records"], want)]


def check_chain(got, m, c):
    check_decode(got, m, c)
    assert not first_bad(got["bits"], m["bits"]), [c["note"][i] for i in first_bad(got["bits"], m["bits"])]
    assert (got["n_env"] == m["n_env"]).all(), (got["n_env"], m["n_env"])
    assert not first_bad(got["env_idx"], m["env_idx"])
    assert (got["envelopes"] == m["envelopes"]).all()
    assert (got["signers"] == m["signers"]).all() and (got["counts"] == m["counts"]).all()
    assert not first_bad(got["certs"], m["certs"]), (got["certs"][:4], m["certs"][:4])


def against_decode_reply(c, heads):
    """Reply by reply: the device's head is pbft_wire_decode_reply's, with the signer's and the client's rule on top."""
    w = A.world()
    for i, t in enumerate(c["texts"]):
        h, g = wire.decode_reply(t), heads[i]
        if not c["inside"][i] or int(h["status"]) != wire.RH_OK:
            assert int(g["status"]) == wire.ACCEPT_EDEFER, (i, c["note"][i])
            continue
        rep = int(h["replica"])
        st = (wire.ACCEPT_ESIGNER if rep >= A.N_REPLICAS or bytes(h["peer_id"]) != w.pids[rep] else
              wire.ACCEPT_ECLIENT if int(c["client_idx"][i]) >= len(A.CLIENTS) else wire.ACCEPT_OK)
        assert int(g["status"]) == st, (i, c["note"][i])
        if st == wire.ACCEPT_OK:
            assert tuple(int(g[k]) for k in ("view", "timestamp", "result_off", "result_len", "replica")) == \
                tuple(int(h[k]) for k in ("view", "timestamp", "result_off", "result_len", "replica"))


# ---- 1. stage (a) ----
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 130])
def test_decode_exact(av, n):
    c = A.prefix(A.corpus(17), n)
    m = A.model(c, settle=False)
    got = run_device(av, A.pack(c), c["client_idx"], chain=False)
    check_decode(got, m, c)
    against_decode_reply(c, got["heads"])
    if n == 130:
        lens = {int(h["result_len"]) for h in got["heads"] if int(h["status"]) == 0}
        assert lens >= set(A.RES_LENS)  # the hash's block boundaries


# ---- 2. alignments ----
@pytest.mark.parametrize("shift", range(16))
def test_every_alignment_of_the_texts(av, shift):
    """The first text at `shift` mod 16 and, with a gap of shift % 5 bytes behind every text, each text at every
    alignment mod 4; the buffer ends at text_bytes = 1, 2, 3 mod 4 (shift % 3 + 1) with poison behind it and in
    every gap, none of which may enter a head, a record or D."""
    c = A.prefix(A.corpus(17, with_outside=False), 65)
    m = A.model(c, settle=False)
    _, off, lens, _ = A.pack(c, gap=shift % 5)
    off = off + np.uint64(shift)
    last = int(np.argmax(off))
    off[last] += np.uint64((shift % 3 + 1 - int(off[last]) - int(lens[last])) % 4)
    tb = int(off[last]) + int(lens[last])
    assert tb % 4 == shift % 3 + 1 and int(off.min()) == shift and {int(o) % 4 for o in off} == {0, 1, 2, 3}
    buf = np.full((tb + 15) // 16 * 16 + 32, POISON, np.uint8)
    for o, t in zip(off, c["texts"]):
        buf[int(o):int(o) + len(t)] = np.frombuffer(t, np.uint8)
    got = run_device(av, (buf, off, lens, tb), c["client_idx"], chain=False)
    check_decode(got, m, c)


def test_texts_outside_text_bytes(av):
    c = A.corpus(17)
    out = [i for i, k in enumerate(c["inside"]) if not k]
    assert out
    m = A.model(c, settle=False)
    got = run_device(av, A.pack(c), c["client_idx"], chain=False)
    for i in out:
        assert int(got["heads"][i]["status"]) == wire.ACCEPT_EDEFER and not got["records"][i][:150].any()
    check_decode(got, m, c)
    # text_bytes one byte short of the last text: that text is outside now, and only that one changes
    buf, off, lens, tb = A.pack(c)
    ins = np.array(c["inside"])
    last = int(np.argmax(np.where(ins, off + lens, 0)))
    c2 = dict(c, inside=[k and i != last for i, k in enumerate(c["inside"])])
    got = run_device(av, (buf, off, lens, tb - 1), c["client_idx"], chain=False)
    check_decode(got, A.model(c2, settle=False), c2)


# ---- 3. the chain ----
@pytest.mark.parametrize("n", [0, 1, 64, 130])
def test_chain_exact(av, n):
    c = A.prefix(A.corpus(17), n)
    m = A.model(c, settle=False)
    got = run_device(av, A.pack(c), c["client_idx"])
    check_chain(got, m, c)
    if n == 130:
        ne = int(m["n_env"][0])
        acc = m["certs"]["accepted"][:ne].astype(bool)
        assert acc.sum() >= 10 and (~acc).sum() >= 5 and (got["certs"]["first"][ne:] == NONE).all()


@pytest.mark.parametrize("env_cap", [1, 7, 27, 28, 29])
def test_short_envelope_table_loses_and_never_miscounts(av, env_cap):
    c = A.corpus(17)
    full = A.model(c, settle=False)
    assert int(full["n_env"][0]) == 28
    m = A.model(c, settle=False, env_cap=env_cap)
    got = run_device(av, A.pack(c), c["client_idx"], env_cap=env_cap)
    check_chain(got, m, c)
    k = min(env_cap, 28)
    assert (got["counts"][:k] == full["counts"][:k]).all() and not first_bad(got["certs"][:k], full["certs"][:k])
    assert int(got["n_env"][1]) == int((full["env_idx"] >= env_cap).sum() - (full["env_idx"] == NONE).sum())


def test_need_is_the_threshold(av):
    c = A.corpus(17)
    for need in (1, 3, 4):
        m = A.model(c, settle=False, need=need)
        got = run_device(av, A.pack(c), c["client_idx"], need=need)
        assert not first_bad(got["certs"], m["certs"])
    assert 0 < int(A.model(c, settle=False, need=4)["certs"]["accepted"].sum()) < \
        int(A.model(c, settle=False, need=1)["certs"]["accepted"].sum())


# ---- 4. the blocking form ----
def test_blocking_form_on_the_mixed_batch(av):
    c = A.corpus(85, with_outside=False)
    n = len(c["texts"])
    m = A.model(c, settle=True, env_cap=128)
    got = av.accept_replies(wire.pack_replies(c["texts"]), A.CLIENTS, A.NEED, 128, client_idx=c["client_idx"])
    st = [int(s) & 0xFF for s in got["heads"]["status"]]
    assert wire.ACCEPT_EDEFER not in st and st.count(wire.ACCEPT_EJSON) >= 2
    assert sum(1 for s in got["heads"]["status"] if int(s) & wire.ACCEPT_ESCAPED) >= 8
    got["bits"] = np.unpackbits(got["bitmap"].view(np.uint8), bitorder="little")[:n].astype(bool)
    assert not first_bad(got["heads"], m["heads"]), [c["note"][i] for i in first_bad(got["heads"], m["heads"])]
    assert not first_bad(got["bits"], m["bits"]), [c["note"][i] for i in first_bad(got["bits"], m["bits"])]
    assert (got["n_env"] == m["n_env"]).all() and not first_bad(got["env_idx"], m["env_idx"])
    assert (got["envelopes"] == m["envelopes"]).all() and (got["signers"] == m["signers"]).all()
    assert (got["counts"] == m["counts"]).all() and not first_bad(got["certs"], m["certs"])
    # the general results are decided like any other: all four replicas' replies in one accepted envelope
    gen = [i for i, x in enumerate(c["note"]) if x == "general"]
    assert len(gen) == 16 and all(got["bits"][i] for i in gen)
    assert all(int(got["certs"][int(got["env_idx"][i])]["count"]) == 4 for i in gen)
    # an empty batch, and no env_idx
    e = av.accept_replies(wire.pack_replies([]), A.CLIENTS, A.NEED, 3)
    assert list(e["n_env"]) == [0, 0] and list(e["certs"]["first"]) == [NONE] * 3 and not e["counts"].any()
    assert av.accept_replies(wire.pack_replies(c["texts"][:9]), A.CLIENTS, A.NEED, 9, client_idx=c["client_idx"][:9],
                             want_env_idx=False)["env_idx"] is None


# ---- 5. capture and replay ----
def test_capture_and_replay(av):
    """The chain as one hipGraph over three loads of one shape (the corpus in three orders)."""
    import torch
    dev = torch.device("cuda", 0)
    probe_t = torch.zeros(16, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    try:
        with torch.cuda.graph(torch.cuda.CUDAGraph()):
            probe_t.add_(1)
    except RuntimeError as e:
        pytest.skip("stream capture refused: %s" % e)
    base = A.corpus(17, with_outside=False)
    n = len(base["texts"])

    def reorder(idx):
        return dict(texts=[base["texts"][i] for i in idx], client_idx=base["client_idx"][idx].copy(),
                    inside=[True] * n, note=[base["note"][i] for i in idx])
    loads = [reorder(np.arange(n)), reorder(np.arange(n)[::-1]), reorder(np.roll(np.arange(n), 37))]
    packs = [A.pack(c) for c in loads]
    tb = packs[0][3]
    assert all(p[3] == tb and len(p[0]) == len(packs[0][0]) for p in packs)
    cap, W = n, 1
    av.accept_reserve(n), av.reserve(n), av.group_reserve(n)
    d_in = [torch.zeros(s, dtype=torch.uint8, device=dev) for s in (len(packs[0][0]), 8 * n, 4 * n, 4 * n)]
    d_cl = torch.from_numpy(clients_table()).to(dev)
    sizes = dict(records=160 * n, heads=32 * n, bitmap=8 * ((n + 63) // 64), env_idx=4 * n, envelopes=85 * cap + 3,
                 n_env=8, signers=8 * cap * W, counts=4 * cap, certs=32 * cap)
    d = {k: torch.zeros(s, dtype=torch.uint8, device=dev) for k, s in sizes.items()}
    p = [t.data_ptr() for t in d_in]
    args = (p[0], tb, p[1], p[2], d_cl.data_ptr(), len(A.CLIENTS), n, A.NEED, d["records"].data_ptr(),
            d["heads"].data_ptr(), d["bitmap"].data_ptr(), cap, d["env_idx"].data_ptr(), d["envelopes"].data_ptr(),
            d["n_env"].data_ptr(), d["signers"].data_ptr(), d["counts"].data_ptr(), d["certs"].data_ptr())

    def load(k):
        buf, off, lens, _ = packs[k]
        for t, a in zip(d_in, (buf, off, lens, loads[k]["client_idx"])):
            t.copy_(torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()))

    load(0)
    av.accept_replies_device(*args, d_client_idx=p[3])  # (an eager call first: the kernels are loaded)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):  # (an error of the call under capture fails the test)
        av.accept_replies_device(*args, d_client_idx=p[3], stream=torch.cuda.current_stream().cuda_stream)
    for k in (1, 2, 0):
        load(k)
        for t in d.values():
            t.fill_(POISON)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        raw = {key: t.cpu().numpy() for key, t in d.items()}
        got = dict(records=raw["records"].reshape(n, 160), heads=raw["heads"].view(wire.AcceptHead),
                   bits=np.unpackbits(raw["bitmap"], bitorder="little")[:n].astype(bool),
                   env_idx=raw["env_idx"].view(np.uint32), envelopes=raw["envelopes"][:85 * cap].reshape(cap, 85),
                   n_env=raw["n_env"].view(np.uint32), signers=raw["signers"].view(np.uint64).reshape(cap, W),
                   counts=raw["counts"].view(np.uint32), certs=raw["certs"].view(wire.AcceptCert))
        check_chain(got, A.model(loads[k], settle=False), loads[k])
        assert (raw["envelopes"][85 * cap:] == POISON).all()


# ---- 6. end to end with the library's signer ----
def test_end_to_end_with_the_library_signer(av):
    """One context signs as each of the four replicas in turn (pbft_sign_replies); the client accepts every request,
    and `first` points at a text that holds the right result.  With one replica's results altered it still does; with
    three altered, each differently, it accepts nothing."""
    from pbft_amd import GpuBatchVerifier
    res, ts, cl = A.R.mixed_results(22, salt=1)
    ts = [1 + 3 * i for i in range(22)]  # one request per timestamp
    table = sorted(set(cl))
    ci = [table.index(x) for x in cl]
    s = GpuBatchVerifier(0)
    try:
        def texts_of(replica, results):
            assert s.set_signing_seed(A.SEEDS[replica], replica).tobytes() == A.world().pubs[replica]
            stream, off, _, _, _ = s.sign_replies(5, wire.pack_results(results, ts, cl))
            return [stream[int(off[i]):int(off[i + 1])].tobytes() for i in range(22)]
        honest = [texts_of(r, res) for r in range(4)]
        bad = [texts_of(r, [x[:3000] + b"%d" % r for x in res]) for r in range(4)]
    finally:
        s.close()

    def accept(per_replica):
        texts = [t for i in range(22) for t in (p[i] for p in per_replica)]
        idx = np.repeat(np.array(ci, np.uint32), 4)
        got = av.accept_replies(wire.pack_replies(texts), table, A.NEED, 128, client_idx=idx)
        return texts, got

    def decided(texts, got):
        out = {}
        for e in range(int(got["n_env"][0])):
            c = got["certs"][e]
            if int(c["accepted"]):
                h, r = wire.decode_reply_json(texts[int(c["first"])])
                out[(int(c["timestamp"]), int(c["client"]))] = r
        return out
    for alter in ([], [2]):
        texts, got = accept([bad[r] if r in alter else honest[r] for r in range(4)])
        d = decided(texts, got)
        assert d == {(ts[i], ci[i]): res[i] for i in range(22)}
        assert int(got["n_env"][0]) == 22 * (1 + len(alter)) and sorted(got["counts"][:22 * (1 + len(alter))])[-22:] == \
            [4 - len(alter)] * 22
    texts, got = accept([bad[r] if r != 0 else honest[r] for r in range(4)])
    assert decided(texts, got) == {} and int(got["n_env"][0]) == 88 and (got["counts"][:88] == 1).all()


# ---- 7. arguments ----
def test_arguments(av):
    from pbft_amd import GpuBatchVerifier, PbftError
    c = A.prefix(A.corpus(17), 9)
    packed = A.pack(c)

    def code(fn, *a, **kw):
        with pytest.raises(PbftError) as e:
            fn(*a, **kw)
        return e.value.code
    bare = GpuBatchVerifier(0)
    try:  # no key set
        assert code(bare.accept_reserve, 16) == -3
        assert code(bare.accept_replies, wire.pack_replies(c["texts"]), A.CLIENTS, A.NEED, 16) == -3
        assert code(run_device, bare, packed, c["client_idx"]) == -3
    finally:
        bare.close()
    assert code(run_device, av, packed, c["client_idx"], need=0) == -1
    assert code(av.accept_replies, wire.pack_replies(c["texts"]), A.CLIENTS, 0, 16) == -1
    assert code(av.accept_replies, wire.pack_replies(c["texts"]), A.CLIENTS, A.NEED, 0) == -1  # env_cap = 0
    assert code(run_device, av, packed, c["client_idx"], env_cap=0) == -1
    assert code(av.accept_reserve, 2**24 + 1) == -1
    # a text outside text_bytes: the blocking form refuses the call
    buf, off, lens = wire.pack_replies(c["texts"])
    assert code(av.accept_replies, (buf, off, lens), A.CLIENTS, A.NEED, 16, text_bytes=int(lens.sum()) - 1) == -1
    # N > 2^24, text_bytes > 2^31 and misaligned pointers: refused before anything is used
    import torch
    mem = torch.zeros(1 << 20, dtype=torch.uint8, device=torch.device("cuda", 0))
    a = mem.data_ptr()  # (real memory, although a refused call touches none of it)
    assert a % 256 == 0
    dev_args = lambda **kw: dict(dict(d_text=a, text_bytes=4096, d_off=a, d_len=a, d_clients=a, n_clients=3, n=9,  # noqa: E731
                                      need=2, d_records=a, d_heads=a, d_bitmap=a, env_cap=9, d_env_idx=a, d_envelopes=a,
                                      d_n_env=a, d_signers=a, d_count=a, d_certs=a), **kw)
    for kw in (dict(n=2**24 + 1), dict(text_bytes=2**31 + 1), dict(d_text=a + 8), dict(d_off=a + 4), dict(d_len=a + 2),
               dict(d_records=a + 8), dict(d_heads=a + 4), dict(d_bitmap=a + 4), dict(d_env_idx=a + 2),
               dict(d_n_env=a + 2), dict(d_signers=a + 4), dict(d_count=a + 2), dict(d_certs=a + 8),
               dict(d_client_idx=a + 2), dict(d_records=0), dict(d_certs=0), dict(d_n_env=0)):
        assert code(av.accept_replies_device, **dev_args(**kw)) == -1, kw
    # a clone shares the key set but has no table of its own until it reserves one
    cl = av.clone()
    try:
        assert code(run_device, cl, packed, c["client_idx"]) == -1
        cl.accept_reserve(16)
        check_chain(run_device(cl, packed, c["client_idx"]), A.model(c, settle=False), c)
    finally:
        cl.close()


# ---- 8. key-set changes ----
def test_key_set_changes():
    from pbft_amd import GpuBatchVerifier, PbftError
    w = A.world()
    new_seed = hashlib.sha512(b"accept-replica-2-renewed").digest()[:32]
    new_pub = A.R.public_key(w.o, new_seed)
    new_pid = wire.peer_id_b58(new_pub)

    def mk(signer_seed, pid, ts, claim=2):
        return A.text_of(1, ts, b"awesome!", claim, pid, w.sign(signer_seed, A.envelope(1, ts, A.CLIENTS[0], b"awesome!")))
    texts = [mk(A.SEEDS[2], w.pids[2], 7), mk(new_seed, new_pid, 7), A.reply(w, 0, 1, 7, 0, b"awesome!"),
             mk(new_seed, w.pids[2], 7), mk(A.SEEDS[2], new_pid, 7)]
    c = dict(texts=texts, client_idx=np.zeros(5, np.uint32), inside=[True] * 5, note=["old", "new", "r0", "mix", "mix"])
    v = GpuBatchVerifier(0)
    try:
        assert v.set_keys(w.keys).all()
        v.accept_reserve(8)
        m = A.model(c, settle=False)
        assert [int(s) for s in m["heads"]["status"]] == [0, 2, 0, 0, 2] and list(m["bits"]) == [True, False, True, False, False]
        assert int(m["certs"][0]["accepted"]) == 1 and int(m["certs"][0]["first"]) == 0
        check_chain(run_device(v, A.pack(c), c["client_idx"]), m, c)
        assert v.update_keys([2], np.frombuffer(new_pub, np.uint8).reshape(1, 32)).all()
        with pytest.raises(PbftError) as e:  # the table is stale: the device form refuses
            run_device(v, A.pack(c), c["client_idx"])
        assert e.value.code == -1
        pubs, pids = list(w.pubs), list(w.pids)
        pubs[2], pids[2] = new_pub, new_pid
        m = A.model(c, settle=False, pids=pids, verify=w.verify_with(pubs))
        assert [int(s) for s in m["heads"]["status"]] == [2, 0, 0, 2, 0] and list(m["bits"]) == [False, True, True, False, False]
        assert int(m["certs"][0]["accepted"]) == 1 and int(m["certs"][0]["first"]) == 1
        # the blocking form rebuilds the table itself; the device form after accept_reserve
        got = v.accept_replies(wire.pack_replies(texts), A.CLIENTS, A.NEED, 5)
        assert not first_bad(got["heads"], m["heads"]) and not first_bad(got["certs"], A.model(
            c, settle=True, pids=pids, verify=w.verify_with(pubs))["certs"])
        v.accept_reserve(8)
        check_chain(run_device(v, A.pack(c), c["client_idx"]), m, c)
        # a new key set of another size
        assert v.set_keys(w.keys[:2]).all()
        v.accept_reserve(8)
        m = A.model(c, settle=False, pids=w.pids[:2], verify=w.verify_with(w.pubs[:2]))
        assert [int(s) for s in m["heads"]["status"]] == [2, 2, 0, 2, 2]
        check_chain(run_device(v, A.pack(c), c["client_idx"]), m, c)
    finally:
        v.close()
