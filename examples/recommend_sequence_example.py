"""Continue a history by several items, each one conditioned on the ones before (a queue, "watch these three next"): load a saved
model (run bert4rec_ml_1m_example.py or bert4rec_lifecycle_example.py first), then ask the app for the greedy continuation, the most
probable continuations by beam search and two sampled continuations.  The items are appended on the GPU between the forwards
(Recommender.recommend_sequences); nothing is read back between the steps."""
import argparse
import math
import pathlib

from _common import dataloaders, datasets, models

from bert4rec_amd.apps import Recommender
from bert4rec_amd.models import model_utils

if __name__ == "__main__":
    parser = argparse.ArgumentParser(description=__doc__)
    parser.add_argument("model", nargs="?", default="bert4rec_ml-1m_lifecycle")
    parser.add_argument("--steps", type=int, default=3)
    parser.add_argument("--beams", type=int, default=3)
    parser.add_argument("--sample", type=int, default=7, help="seed of the sampled continuations")
    args = parser.parse_args()
    path = model_utils.determine_model_path(pathlib.Path(args.model))
    loaded = models.BERT4RecModelWrapper.load(path)
    kwargs = {"tokenizer": loaded["tokenizer"]} if "tokenizer" in loaded else {}
    if not datasets.ML1M.is_available():
        kwargs["data_source"] = datasets.synthetic_dataset(n_users=1500, n_items=3706, min_len=20, max_len=200, seed=0, order=0.6)
    dataloader = dataloaders.get_dataloader_factory("bert4rec").create_ml_1m_dataloader(**kwargs)
    dataloader.generate_vocab()
    app = Recommender(loaded["model_wrapper"].model, dataloader)
    history = dataloader.get_tokenizer().detokenize([7, 19, 4, 33, 12])
    print("history:", history)
    print("next %d items, greedy:" % args.steps, app.recommend_sequences([history], args.steps)[0])
    print("with the probability of every step:", app.recommend_sequences([history], args.steps, return_probabilities=True)[0])
    for items, logp in app.recommend_sequences([history], args.steps, beams=args.beams)[0]:
        print("beam, probability %.3g:" % math.exp(logp), items)
    # two simulated continuations of the same user: the user repeated under two noise streams
    for stream, items in enumerate(app.recommend_sequences([history, history], args.steps, sample_seed=args.sample, user_streams=[0, 1])):
        print("drawn continuation %d:" % stream, items)
