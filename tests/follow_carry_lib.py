"""The follow path on carry sessions (CEP_SESSION_FOLLOW_CARRY, test_follow_carry_cpu.py,
test_follow_carry_gpu.py): a Python restatement of the carried walks as a reference model, the
oracle's per-batch expectation, and stream generators.

A batch is a dict: key (grouped), val, topic (or None), pos (the records' stream positions)."""
import struct

import numpy as np

import oracle as O
import follow_lib as FL

DEAD, DONE, OPEN = 0, 1, 2


def _steps(nslots, is_next, ok, p, s0, end):
    """a walk continued at slot s0 from record p inside the key segment ending at `end`:
    (outcome, slots reached, records taken from s0 on)"""
    taken = []
    for s in range(s0, nslots):
        if is_next[s]:
            while p < end and not ok(s, p):
                p += 1
        if p >= end:
            return OPEN, s, taken
        if not ok(s, p):
            return DEAD, s, taken
        taken.append(p)
        p += 1
    return DONE, nslots, taken


def carried_model(stages, batches):
    """per batch the matches (record position, key, traversal), in the order the session emits them:
    by completing record of the grouped batch, a key's carried walks (in list order) before its in-batch ones"""
    slots, owner = FL.slots_of(stages)
    K = len(slots)
    is_next = [nx for _, nx in slots]
    state = {}                                           # key -> [[s, pos_0 .. pos_(s-1)], ...] in ascending start
    res = []
    for b in batches:
        key, pos = np.asarray(b["key"]), np.asarray(b["pos"])
        n = len(key)
        hits = [FL.stage_hits(st, b["val"], b["topic"]) for st in stages]
        ok = lambda s, p: bool(hits[owner[s]][p])
        starts = [i for i in range(n) if i == 0 or key[i] != key[i - 1]] + [n]
        done = []                                        # (completing record, run, order within the run, match)
        new_state = {}
        for sg in range(len(starts) - 1):
            a, e = starts[sg], starts[sg + 1]
            k = int(key[a])
            assert k not in new_state, "a key in two segments"
            walks = state.get(k, [])
            # one continuation per slot, whatever the number of walks waiting at it
            cont = {s: _steps(K, is_next, ok, a, s, e) for s in range(1, K)} if walks else {}
            lst = []
            for w in walks:
                s = w[0]
                out, reached, taken = cont[s]
                recs = w[1:1 + s] + [int(pos[t]) for t in taken]
                if out == DONE:
                    done.append((taken[-1], 0, len(done), (k, recs)))
                elif out == OPEN:
                    lst.append([reached] + recs)
            for j0 in range(a, e):
                if not ok(0, j0):
                    continue
                out, reached, taken = _steps(K, is_next, ok, j0 + 1, 1, e)
                recs = [int(pos[j0])] + [int(pos[t]) for t in taken]
                if out == DONE:
                    done.append((taken[-1], 1, j0, (k, recs)))
                elif out == OPEN:
                    lst.append([reached] + recs)
            new_state[k] = lst
        for k, lst in new_state.items():                 # a key absent from the batch keeps its list
            state[k] = lst
        # the two runs (carried, then in-batch), stably sorted on the completing record only
        done.sort(key=lambda t: (t[1], t[2]))
        done.sort(key=lambda t: t[0])
        res.append([(recs[-1], k, [(slots[s][0], r) for s, r in reversed(list(enumerate(recs)))])
                    for _, _, _, (k, recs) in done])
    return res, state


def oracle_batches(stages, schema, batches, mode=O.MODE_NFA_PER_KEY, by_position=True):
    """the oracle over every key's whole stream, its records mapped to their stream positions: per batch the
    matches completing in it, by (completing record's place in the batch, start)"""
    ir = FL.build(stages).to_ir(schema)
    per_key = {}
    for bi, b in enumerate(batches):
        for i, k in enumerate(np.asarray(b["key"])):
            per_key.setdefault(int(k), []).append((bi, i))
    keys = sorted(per_key)
    if not keys:
        return [[] for _ in batches]
    flat = [(k, bi, i) for k in keys for bi, i in per_key[k]]
    key = np.array([k for k, _, _ in flat], np.int32)
    val = np.array([batches[bi]["val"][i] for _, bi, i in flat], np.int32)
    with_topic = any(b["topic"] is not None for b in batches)
    topic = np.array([batches[bi]["topic"][i] for _, bi, i in flat], np.int32) if with_topic else None
    p = O.OraclePattern(ir)
    r = O.OracleRun(p, mode)
    r.process(O.BatchArrays(key, [val], [1], topic=topic))
    out = [[] for _ in batches]
    for m in r.matches(with_groups=False):
        _, bi, i = flat[m.record]
        posn = lambda rec: int(batches[flat[rec][1]]["pos"][flat[rec][2]])
        trav = [(p.names[nm], posn(ev)) for nm, ev in m.traversal]
        out[bi].append((i, trav[-1][1], (posn(m.record), int(m.key), trav)))
    return [[t[2] for t in sorted(lst, key=lambda t: (t[0], t[1]))] for lst in out]


def split_stream(rng, n_keys, max_len, alphabet, n_batches, min_len=1):
    """n_keys keys of min_len..max_len records, each key's stream cut at n_batches - 1 random points of its own
    (a cut may repeat: the key is then absent from a batch); per batch the grouped arrays and positions"""
    lens = rng.integers(min_len, max_len + 1, n_keys)
    pieces = []
    for k in range(n_keys):
        cuts = np.sort(rng.integers(0, lens[k] + 1, n_batches - 1))
        pieces.append(np.diff(np.concatenate([[0], cuts, [lens[k]]])))
    batches, base = [], 0
    for bi in range(n_batches):
        cnt = np.array([pieces[k][bi] for k in range(n_keys)], np.int64)
        key = np.repeat(np.arange(n_keys, dtype=np.int32), cnt)
        n = len(key)
        batches.append(dict(key=key, val=rng.integers(0, alphabet, n).astype(np.int32),
                            topic=rng.integers(0, 2, n).astype(np.int32), pos=base + np.arange(n, dtype=np.int64)))
        base += n
    return batches


def batches_of(parts):
    """parts: per batch a list of (key, values); positions follow the batches"""
    out, base = [], 0
    for part in parts:
        key = np.concatenate([np.full(len(v), k, np.int32) for k, v in part] or [np.zeros(0, np.int32)])
        val = np.concatenate([np.asarray(v, np.int32) for _, v in part] or [np.zeros(0, np.int32)])
        out.append(dict(key=key, val=val, topic=None, pos=base + np.arange(len(key), dtype=np.int64)))
        base += len(key)
    return out


def walk_blob(k, next_pos, keys, magic=b"KCSW", version=1):
    """a state blob by hand: keys = [(key id, [[s, pos ...], ...])], walks padded to k words"""
    out = bytearray(magic + struct.pack("<IqI", version, next_pos, len(keys)))
    for kid, walks in keys:
        out += struct.pack("<iiii", kid, len(walks), k, 0)
        for w in walks:
            out += struct.pack("<%dq" % k, *(list(w) + [0] * (k - len(w))))
    return bytes(out)
