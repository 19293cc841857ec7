"""The logistic-normal topic model trained by Monte Carlo EM.

Counterpart of the reference's examples/topic_models/lntm_mcem.py, whose ``LNTM.forward`` is ``pass``, written out as its
tutorial (docs/tutorials/lntm.rst) describes the model: ``eta ~ Normal(eta_mean, exp(eta_logstd))`` per document,
``theta = softmax(eta)``, ``phi = softmax(beta)`` per topic and the words ``x ~ UnnormalizedMultinomial(log(theta @ phi))`` --
here the ``admixture_multinomial`` node, whose value and gradients come from the matrix-core kernels of include/zs_topic.h
without the ``[chains x documents, words]`` product ever reaching memory.

E-step: HMC over ``eta`` on ``n_chains`` chains per document (every (chain, document) pair is a chain of the sampler), the step
size adapting towards an acceptance rate of 0.6; then the closed-form update of ``eta_mean`` / ``eta_logstd`` from the samples.
M-step: one Adam step on ``beta`` with the likelihood averaged over the chains.  The corpus is synthetic, drawn from the model
itself: no dataset, no download."""
import argparse

import torch

from zhusuan.framework.bn import BayesianNet
from zhusuan.mcmc import HMC


class LNTM(BayesianNet):
    def __init__(self, n_chains, n_docs, n_topics, n_words, device):
        super().__init__()
        self.eta_shape = (n_chains, n_docs, n_topics)
        self.freeze_topics = False          # the E-step: beta (topic_logits) is a constant, so its gradient kernels are not launched
        self.topic_logits = torch.nn.Parameter(torch.zeros(n_topics, n_words))
        self.register_buffer('eta_mean', torch.zeros(n_topics))
        self.register_buffer('eta_logstd', torch.zeros(n_topics))
        self.to(device)

    def forward(self, observed):
        self.observe(observed)
        # x [n_docs, n_words] is shared by the chains
        eta = self.normal('eta', mean=self.eta_mean.expand(self.eta_shape).contiguous(),
                          logstd=self.eta_logstd.expand(self.eta_shape).contiguous(), group_ndims=1)
        self.admixture_multinomial('x', eta, self.topic_logits.detach() if self.freeze_topics else self.topic_logits)
        return self


def synthetic_corpus(n_docs, n_topics, n_words, doc_len, seed):
    """Counts [n_docs, n_words] drawn from the model with beta ~ 2 N(0, 1) and eta ~ N(0, 1) (host generator: reproducible)."""
    gen = torch.Generator().manual_seed(seed)
    phi = torch.softmax(2.0 * torch.randn(n_topics, n_words, generator=gen), -1)
    theta = torch.softmax(torch.randn(n_docs, n_topics, generator=gen), -1)
    words = torch.multinomial(theta @ phi, doc_len, replacement=True, generator=gen)
    return torch.zeros(n_docs, n_words).scatter_add_(1, words, torch.ones(n_docs, doc_len))


def run(n_chains=4, n_docs=32, n_topics=5, n_words=200, doc_len=80, n_rounds=20, hmc_iters=3, n_leapfrogs=5, lr=0.1,
        device='cuda', seed=1, log=None):
    """``n_rounds`` EM rounds.  Returns a dict: ``per_word_ll`` (one float per round: the chain-averaged log-likelihood per word
    after the E-step), ``acceptance`` (mean acceptance rate of the last round), ``step_size``, and the device tensors ``beta``
    [n_topics, n_words], ``eta`` [n_chains, n_docs, n_topics], ``eta_mean`` and ``eta_logstd`` [n_topics]."""
    device = torch.device(device)
    if device.type == 'cuda':
        torch.cuda.manual_seed(seed)
    x = synthetic_corpus(n_docs, n_topics, n_words, doc_len, seed).to(device)
    n_tokens = float(x.sum())
    model = LNTM(n_chains, n_docs, n_topics, n_words, device)
    sampler = HMC(step_size=0.05, n_leapfrogs=n_leapfrogs, adapt_step_size=True, target_acceptance_rate=0.6)
    opt = torch.optim.Adam([model.topic_logits], lr=lr)
    eta = torch.zeros(n_chains, n_docs, n_topics, device=device)
    per_word, rate = [], 0.0
    for rnd in range(n_rounds):
        # E-step: HMC over eta with beta fixed, then the closed-form Gaussian fit of the samples
        rate = 0.0
        model.freeze_topics = True
        for _ in range(hmc_iters):
            latent, info = sampler.sample(model, {'x': x}, {'eta': eta})
            eta = latent['eta']
            rate += float(info.acceptance_rate.mean()) / hmc_iters
        flat = eta.reshape(-1, n_topics)
        model.eta_mean.copy_(flat.mean(0))
        model.eta_logstd.copy_(torch.log(flat.std(0, unbiased=False) + 1e-3))
        # M-step: one Adam step on beta, the likelihood averaged over the chains
        model.freeze_topics = False
        opt.zero_grad()
        model({'eta': eta, 'x': x})
        ll = model.nodes['x'].log_prob().mean(0).sum()
        (-ll / n_tokens).backward()
        opt.step()
        per_word.append(float(ll.detach()) / n_tokens)
        if log:
            log("round %d  per-word log-likelihood %.4f  acceptance %.3f  step size %.4f" % (rnd + 1, per_word[-1], rate, sampler.step_size))
    return dict(per_word_ll=per_word, acceptance=rate, step_size=sampler.step_size, beta=model.topic_logits.detach(), eta=eta,
                eta_mean=model.eta_mean, eta_logstd=model.eta_logstd)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--chains', type=int, default=4)
    ap.add_argument('--docs', type=int, default=32)
    ap.add_argument('--topics', type=int, default=5)
    ap.add_argument('--words', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=20)
    args = ap.parse_args()
    r = run(n_chains=args.chains, n_docs=args.docs, n_topics=args.topics, n_words=args.words, n_rounds=args.rounds, log=print)
    print('per-word log-likelihood: first round %.4f, last round %.4f (uniform words: %.4f)'
          % (r['per_word_ll'][0], r['per_word_ll'][-1], -torch.log(torch.tensor(float(args.words)))))


if __name__ == '__main__':
    main()
