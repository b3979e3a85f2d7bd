"""Recommend the next item for a history (the reference's examples/recommender_app_example.py): load a saved model (run
bert4rec_ml_1m_example.py or bert4rec_lifecycle_example.py first), then ask the app.
--diversity D (0 .. 1) also prints a top 5 re-ranked for diversity (greedy Maximal Marginal Relevance over the 50 best candidates).
--sample SEED also prints 5 items drawn from the softmax over the 50 best candidates, with the probability of each."""
import argparse
import pathlib

from _common import dataloaders, datasets, models

from bert4rec_amd.apps import Recommender
from bert4rec_amd.models import model_utils

if __name__ == "__main__":
    parser = argparse.ArgumentParser(description=__doc__)
    parser.add_argument("model", nargs="?", default="bert4rec_ml-1m_lifecycle")
    parser.add_argument("--diversity", type=float, default=None, help="0 = the plain top k ... 1 = dissimilarity alone")
    parser.add_argument("--sample", type=int, default=None, help="seed of a sampled top 5 (exploration traffic)")
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
    print("next item:", app(history), " top 5:", app(history, k=5))
    if args.diversity is not None:
        print("top 5 at diversity %g:" % args.diversity, app(history, k=5, diversity=args.diversity))
    if args.sample is not None:
        print("5 items drawn with seed %d:" % args.sample,
              app.recommend_batch([history], k=5, sample_seed=args.sample, user_streams=[0], candidate_pool=50, return_probabilities=True)[0])
