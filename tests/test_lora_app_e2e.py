"""Multi-LoRA through the full HTTP app: the OpenAI ``model`` field routes an
adapter name to its base LLM endpoint and on to the adapter (llama-tiny on
CPU)."""

import json
import os
import sys

import pytest
from fastapi.testclient import TestClient

from clearml_serving_amd.models.llama import PRESETS
from clearml_serving_amd.schemas import ModelEndpoint
from clearml_serving_amd.serving.app import create_app

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                "helpers"))
import lora_util  # noqa: E402


@pytest.fixture()
def lora_client(processor, store, tmp_path):
    from clearml_serving_amd.engines.llm.adapter import LlmPreprocessRequest

    LlmPreprocessRequest._engine_singleton = None
    LlmPreprocessRequest._engines = {}
    model_dir = tmp_path / "model"
    model_dir.mkdir()
    (model_dir / "card.json").write_text(json.dumps({
        "arch": "llama", "preset": "llama-tiny", "num_kv_blocks": 64,
        "block_size": 16, "max_model_len": 128, "device": "cpu"}))
    mcfg = PRESETS["llama-tiny"]
    lora_util.write_adapter(str(model_dir / "adapters" / "sql"), mcfg,
                            lora_util.ALL_LINEAR, seed=1)
    lora_util.write_adapter(str(model_dir / "adapters" / "chat"), mcfg,
                            lora_util.ATTN_ONLY, seed=2)
    rec = store.register_model(name="llama-tiny", project="p",
                               path=str(model_dir))
    processor.add_endpoint(ModelEndpoint(
        engine_type="llm", serving_url="test_llm", model_id=rec.model_id,
        auxiliary_cfg={"lora_modules": [
            {"name": "sql-lora", "path": "adapters/sql"},   # relative to
            {"name": "chat-lora", "path": "adapters/chat"},  # the model dir
        ]}))
    processor.serialize()
    app = create_app(processor=processor, poll_frequency_sec=3600)
    with TestClient(app) as c:
        yield c
    LlmPreprocessRequest._engine_singleton = None
    LlmPreprocessRequest._engines = {}


def _chat(client, model):
    r = client.post("/serve/openai/v1/chat/completions", json={
        "model": model, "max_tokens": 6, "temperature": 0.0,
        "ignore_eos": True,
        "messages": [{"role": "user", "content": "hello"}]})
    assert r.status_code == 200, r.text
    return r.json()


def test_adapter_name_routes_through_the_http_front(lora_client):
    base = _chat(lora_client, "test_llm")
    sql = _chat(lora_client, "sql-lora")
    chat = _chat(lora_client, "chat-lora")
    assert base["model"] == "test_llm"
    assert sql["model"] == "sql-lora" and chat["model"] == "chat-lora"
    # (the byte tokenizer decodes random-init ids lossily, so the routing is
    # read from the engine's counter, not from the texts)
    from clearml_serving_amd.engines.llm.adapter import LlmPreprocessRequest

    engine = LlmPreprocessRequest._engine_singleton
    assert engine.stats["lora_requests"] == 2
    assert engine.lora_bank.names == ["sql-lora", "chat-lora"]

    r = lora_client.post("/serve/openai/v1/models", json={"model": "test_llm"})
    assert r.status_code == 200, r.text
    data = r.json()["data"]
    assert [m["id"] for m in data] == ["test_llm", "sql-lora", "chat-lora"]
    assert all(m["parent"] == "test_llm" for m in data[1:])

    r = lora_client.post("/serve/openai/v1/chat/completions", json={
        "model": "no-such-adapter", "max_tokens": 2,
        "messages": [{"role": "user", "content": "hello"}]})
    assert r.status_code == 404
