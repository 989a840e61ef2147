"""Batching inference server (CPU, llama_test, FastAPI TestClient):
concurrent requests share generate_batch calls, max_batch=1 serves one per
call, stop_token_ids, and failure isolation."""
import threading

import pytest

fastapi = pytest.importorskip("fastapi")

REQS = [
    {"prompt": [1, 2, 3], "max_tokens": 5},
    {"prompt": list(range(10, 27)), "max_tokens": 3},
    {"prompt": [9], "max_tokens": 7},
    {"prompt": list(range(40, 80)), "max_tokens": 4},
]


@pytest.fixture(scope="module")
def model():
    import torch

    from prime_amd.models import build_model

    torch.manual_seed(0)
    m = build_model("llama_test")
    m.eval()
    return m


@pytest.fixture()
def calls(monkeypatch):
    """Wrap the function the app calls; record the batch size of each call."""
    from prime_amd.models import generate as gen_mod

    real = gen_mod.generate_batch
    seen = []

    def counting(model, prompts, *a, **kw):
        seen.append(len(prompts))
        return real(model, prompts, *a, **kw)

    monkeypatch.setattr(gen_mod, "generate_batch", counting)
    return seen


def _client(model, **kw):
    from fastapi.testclient import TestClient

    from prime_amd.serve import create_app

    return TestClient(create_app(model, "llama_test", tokenizer=None, **kw))


def _post_all(client, reqs):
    """Post every request from its own thread, released together."""
    out = [None] * len(reqs)
    gate = threading.Barrier(len(reqs))

    def post(i):
        gate.wait()
        out[i] = client.post("/v1/completions", json=reqs[i])

    ts = [threading.Thread(target=post, args=(i,)) for i in range(len(reqs))]
    for t in ts:
        t.start()
    for t in ts:
        t.join(60)
    return out


@pytest.fixture(scope="module")
def solo(model):
    """What each request returns when it is served alone."""
    c = _client(model, max_batch=1)
    out = []
    for r in REQS:
        resp = c.post("/v1/completions", json=r)
        assert resp.status_code == 200, resp.text
        out.append(resp.json())
    return out


def test_concurrent_requests_share_a_call(model, solo, calls):
    c = _client(model, max_batch=4, batch_window_ms=200.0)
    resps = _post_all(c, REQS)
    for r, want, req in zip(resps, solo, REQS):
        assert r.status_code == 200, r.text
        d = r.json()
        assert d["choices"][0]["text"] == want["choices"][0]["text"]
        assert d["usage"] == want["usage"]
        assert d["usage"]["completion_tokens"] == req["max_tokens"]
    assert sum(calls) == 4 and len(calls) < 4


def test_max_batch_one_serves_one_per_call(model, solo, calls):
    c = _client(model, max_batch=1, batch_window_ms=200.0)
    resps = _post_all(c, REQS)
    for r, want in zip(resps, solo):
        assert r.status_code == 200, r.text
        assert r.json()["choices"][0]["text"] == want["choices"][0]["text"]
    assert calls == [1, 1, 1, 1]


def test_stop_token_ids_and_response_keys(model, solo):
    c = _client(model)
    d0 = solo[2]
    assert set(d0) == {"id", "object", "created", "model", "choices", "usage"}
    assert set(d0["choices"][0]) == {"index", "text", "finish_reason"}
    assert set(d0["usage"]) == {"prompt_tokens", "completion_tokens",
                                "total_tokens"}
    assert d0["choices"][0]["finish_reason"] == "length"
    toks = d0["choices"][0]["text"]
    t = toks[1]
    assert t != toks[0]
    r = c.post("/v1/completions", json={**REQS[2], "stop_token_ids": [t]})
    assert r.status_code == 200, r.text
    d = r.json()
    assert set(d) == set(d0)
    assert d["choices"][0]["finish_reason"] == "stop"
    assert d["choices"][0]["text"] == toks[:2]
    assert d["usage"]["completion_tokens"] == 2


def test_failure_is_reported_and_worker_survives(model, solo, monkeypatch):
    from prime_amd.models import generate as gen_mod

    real = gen_mod.generate_batch
    state = {"fail": True}

    def flaky(*a, **kw):
        if state["fail"]:
            raise RuntimeError("boom")
        return real(*a, **kw)

    monkeypatch.setattr(gen_mod, "generate_batch", flaky)
    c = _client(model, max_batch=3, batch_window_ms=200.0)
    resps = _post_all(c, REQS[:3])
    assert [r.status_code for r in resps] == [500, 500, 500]
    state["fail"] = False
    r = c.post("/v1/completions", json=REQS[0])
    assert r.status_code == 200, r.text
    assert r.json()["choices"][0]["text"] == solo[0]["choices"][0]["text"]


def test_oversize_request_is_rejected_alone(model):
    c = _client(model)
    r = c.post("/v1/completions", json={
        "prompt": [1, 2, 3], "max_tokens": model.cfg.max_seq})
    assert r.status_code == 400
    r = c.post("/v1/completions", json={
        "prompt": [model.cfg.vocab_size], "max_tokens": 2})
    assert r.status_code == 400
