"""Guided decoding through the full HTTP app (llama-tiny on CPU, an
endpoint with ``guided_decoding: true``)."""

import json

import pytest
from fastapi.testclient import TestClient

from clearml_serving_amd.schemas import ModelEndpoint
from clearml_serving_amd.serving.app import create_app

SCHEMA = {"type": "object", "required": ["name", "age"],
          "properties": {"name": {"type": "string", "maxLength": 6},
                         "age": {"type": "string", "pattern": "[0-9]{1,3}"},
                         "admin": {"type": "boolean"}}}


@pytest.fixture()
def guided_client(processor, store, tmp_path):
    from clearml_serving_amd.engines.llm.adapter import LlmPreprocessRequest

    LlmPreprocessRequest._engine_singleton = None
    LlmPreprocessRequest._engines = {}
    card = tmp_path / "card.json"
    card.write_text(json.dumps({
        "arch": "llama", "preset": "llama-tiny", "num_kv_blocks": 64,
        "block_size": 16, "max_model_len": 256, "device": "cpu",
        "guided_decoding": True}))
    rec = store.register_model(name="llama-tiny", project="p",
                               path=str(card))
    processor.add_endpoint(ModelEndpoint(
        engine_type="llm", serving_url="test_llm", model_id=rec.model_id))
    processor.serialize()
    app = create_app(processor=processor, poll_frequency_sec=3600)
    with TestClient(app) as c:
        yield c
    LlmPreprocessRequest._engine_singleton = None
    LlmPreprocessRequest._engines = {}


def valid(doc):
    return (isinstance(doc, dict) and list(doc) == [
        k for k in ("name", "age", "admin") if k in doc]
        and isinstance(doc.get("name"), str) and len(doc["name"]) <= 6
        and isinstance(doc.get("age"), str) and doc["age"].isdigit()
        and 1 <= len(doc["age"]) <= 3
        and isinstance(doc.get("admin", True), bool))


def test_chat_json_schema_response_format(guided_client):
    r = guided_client.post("/serve/openai/v1/chat/completions", json={
        "model": "test_llm", "max_tokens": 80, "temperature": 1.0, "seed": 3,
        "messages": [{"role": "user", "content": "a person as json"}],
        "response_format": {"type": "json_schema", "json_schema": {
            "name": "person", "schema": SCHEMA}}})
    assert r.status_code == 200, r.text
    choice = r.json()["choices"][0]
    assert choice["finish_reason"] == "stop"
    assert valid(json.loads(choice["message"]["content"])), choice


def test_guided_choice_on_completions(guided_client):
    r = guided_client.post("/serve/openai/v1/completions", json={
        "model": "test_llm", "prompt": "pick", "max_tokens": 20,
        "temperature": 0.0, "guided_choice": ["red", "green", "blue"]})
    assert r.status_code == 200, r.text
    choice = r.json()["choices"][0]
    assert choice["text"] in ("red", "green", "blue")
    assert choice["finish_reason"] == "stop"


def test_sse_stream_concatenates_to_a_valid_document(guided_client):
    with guided_client.stream(
            "POST", "/serve/openai/v1/chat/completions", json={
                "model": "test_llm", "max_tokens": 80, "temperature": 0.0,
                "stream": True,
                "messages": [{"role": "user", "content": "json please"}],
                "guided_json": SCHEMA}) as r:
        assert r.status_code == 200
        lines = [ln[6:] for ln in r.iter_lines() if ln.startswith("data: ")]
    assert lines[-1] == "[DONE]"
    chunks = [json.loads(ln) for ln in lines[:-1]]
    text = "".join(c["choices"][0]["delta"]["content"] for c in chunks)
    assert chunks[-1]["choices"][0]["finish_reason"] == "stop"
    assert valid(json.loads(text)), text


def test_bad_grammars_are_422(guided_client):
    recursive = {"$defs": {"node": {"type": "object", "properties": {
        "next": {"$ref": "#/$defs/node"}}}}, "$ref": "#/$defs/node"}
    for extra in ({"guided_json": recursive},
                  {"guided_json": recursive, "stream": True},
                  {"guided_regex": "a(?=b)"},
                  {"guided_regex": "a+", "guided_choice": ["a"]},
                  {"guided_regex": "a+", "ignore_eos": True}):
        r = guided_client.post("/serve/openai/v1/completions", json={
            "model": "test_llm", "prompt": "x", "max_tokens": 4, **extra})
        assert r.status_code == 422, (extra, r.text)
