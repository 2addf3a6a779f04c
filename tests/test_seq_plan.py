"""The plan of `every e1=S[c1], e2=S[c2] [within T]` once the compiler marks it for the adjacent-pair closed form
(compiler.cpp fast_seq_adjacent, two hidden (e1, e2) ordinal refs for the NFA hand-over of device batches): the
query tree sm_compile_dump reports is what it was, and the plan still compiles for and runs on the NFA, whose device
code built for the host (tests/native) must give the oracle's outputs (values and visible refs) for it. The same
streams also tie the adjacent-pair rule of kernels/seq_dev.h to the oracle on the CPU: its numpy statement equals the
oracle's refs tuple for tuple. Test infrastructure: no GPU; `-m "not gpu"`."""
import os
import subprocess

import numpy as np
import pytest

import siddhi_amd
from oracle_lib import OracleApp

HERE = os.path.dirname(os.path.abspath(__file__))
SCHEMA = "define stream StockStream (symbol int, price double, volume long, timestamp long); "
PART = "partition with (symbol of StockStream) begin {q} end;"
SEQ = ("@info(name='q') from every e1=StockStream[price>20], e2=StockStream[{c2}]{within} "
       "select e1.timestamp as i, e2.timestamp as j insert into OutputStream;")
TYPES = ["INT", "DOUBLE", "LONG", "LONG"]


def text(partitioned, within, c2="price>e1.price"):
    q = SEQ.format(c2=c2, within=within)
    return SCHEMA + (PART.format(q=q) if partitioned else q)


def test_compile_dump_unchanged():
    d = siddhi_amd.compile_dump(text(True, " within 1 sec"))
    assert d["queries"] == [] and len(d["partitions"]) == 1
    q = d["partitions"][0]["queries"][0]
    assert d["partitions"][0]["with"] == [{"key": {"var": "symbol"}, "stream": "StockStream"}]
    assert q == {
        "input": "sequence", "insert_into": "OutputStream", "name": "q",
        "select": [{"as": "i", "expr": {"ref": "e1", "var": "timestamp"}},
                   {"as": "j", "expr": {"ref": "e2", "var": "timestamp"}}],
        "state": {"next": [
            {"every": {"filters": [{"cmp": ">", "l": {"var": "price"}, "r": {"const": 20, "type": "INT"}}],
                       "ref": "e1", "stream": "StockStream"}},
            {"filters": [{"cmp": ">", "l": {"var": "price"}, "r": {"ref": "e1", "var": "price"}}],
             "ref": "e2", "stream": "StockStream", "within": 1000}]},
    }


@pytest.fixture(scope="module")
def harness():
    subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "native")])
    from host_harness_lib import HostHarnessApp
    return HostHarnessApp


def stream(n=3000, K=7, seed=3):
    rng = np.random.default_rng(seed)
    sym = rng.integers(0, K, n)
    price = np.round(rng.random(n) * 60.0, 1)
    vol = rng.integers(0, 2000, n)
    ts = np.cumsum(rng.integers(0, 3, n))
    return sym, price, vol, ts


def feed(factory, app_text, rows, flush_every=0):
    a = factory(app_text)
    a.start()
    for i, (t, r) in enumerate(rows):
        a.send("StockStream", t, r, TYPES)
        if flush_every and (i + 1) % flush_every == 0:
            a.flush()
    a.flush()
    out = a.outputs()["streams"].get("OutputStream", [])
    a.close()
    return out


def rule_pairs(sym, price, ts, partitioned, T, c2):
    """The adjacent-pair rule: each event against the previous event of its instance."""
    n = len(ts)
    key = sym if partitioned else np.zeros(n, np.int64)
    order = np.argsort(key, kind="stable")
    same = key[order][1:] == key[order][:-1]
    j, i = order[1:][same], order[:-1][same]
    ok = (price[i] > 20) & c2(i, j)
    if T is not None:
        ok &= ts[j] - ts[i] <= T
    p = np.stack([i[ok], j[ok]], axis=1)
    return p[np.argsort(p[:, 1], kind="stable")]


@pytest.mark.parametrize("c2name", ["gt", "plus_and"])
@pytest.mark.parametrize("within,T", [(" within 5 milliseconds", 5), (" within 0 milliseconds", 0), ("", None)])
@pytest.mark.parametrize("partitioned", [True, False])
def test_sequence_on_the_host_nfa_and_the_rule_equal_the_oracle(harness, partitioned, within, T, c2name):
    sym, price, vol, ts = stream()
    c2s = {"gt": ("price>e1.price", lambda i, j: price[j] > price[i]),
           "plus_and": ("price > e1.price + 5.0 and volume < e1.volume",
                        lambda i, j: (price[j] > price[i] + 5.0) & (vol[j] < vol[i]))}
    c2text, c2fn = c2s[c2name]
    t = text(partitioned, within, c2text)
    rows = [(int(ts[i]), [int(sym[i]), float(price[i]), int(vol[i]), i]) for i in range(len(ts))]
    exp = feed(OracleApp, t, rows)
    assert len(exp) > 5
    np.testing.assert_array_equal(np.array([r[2] for r in exp]).reshape(-1, 2),
                                  rule_pairs(sym, price, ts, partitioned, T, c2fn))
    # the harness dumps every ref of an output record: the select's two, then the hidden (e1, e2) pair, equal here
    vis = lambda out: [[r[0], r[1], r[2][:2]] for r in out]
    got = feed(harness, t, rows)
    assert vis(got) == exp and all(r[2][2:] == r[2][:2] for r in got)
    assert vis(feed(harness, t, rows, flush_every=997)) == exp  # lane state carried across batches
